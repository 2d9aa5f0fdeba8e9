"""`haphic build` on the device: the mirrors of the two functions of scripts/HapHiC_build.py that touch the genome.

    parse_fasta            HapHiC_cluster.py:87-113 (imported by HapHiC_build.py:17)  -> containers.FastaTable over _lib.Fasta
    build_final_scaffolds  HapHiC_build.py:74-179                                     -> both AGP files from arrays on the host, scaffolds.fa by one
                                                                                         hhx_fasta_emit call (csrc/hhx_fasta.hip)

parse_tours :29-57 asks the table `ctg in fa_dict` only, parse_corrected_ctgs, generate_juicebox_script, the argument parser and run() :244-283 stay the
reference's.  What the device does not serve goes to the reference's own function (`_original`, bound by patch.patch_build): a FASTA the reader
refuses (a byte >= 0x80, a sequence line before the first header, a text beyond half of the device's memory) or whose contig names repeat (the
reference's dict keeps the first position and the last sequence); a fa_dict that is no frozen FastaTable; max_width < 1 (range() raises or writes
nothing); Ns < 0; a corrected contig whose name does not read `name:start-end` (the reference's assertion / ValueError is the reference's to raise).
`engine`: a stand-in for _lib.Fasta (the tests' numpy engine, tests/build_cases.py)."""
import logging

import numpy as np

from .containers import FastaTable

logger = logging.getLogger(__name__)


def _sites_of(RE):
    from . import cluster
    return cluster._sites_of(RE)


def parse_fasta(fasta, RE='GATC', keep_letter_case=False, logger=logger, _original=None, _engine=None):
    """parse_fasta() :87-113 -> FastaTable; what the reader refuses -> _original(...)"""
    if _engine is None:
        from . import _lib
        _engine = _lib.Fasta
    try:
        fa = _engine(fasta, keep_letter_case=keep_letter_case)
    except _engine.Unsupported:
        if _original is None:
            raise
        return _original(fasta, RE, keep_letter_case, logger)
    table = FastaTable(fa, _sites_of(RE))
    if len(set(table.names)) != len(table.names):                # fa_dict[ctg] = list() :99 on a name seen before
        fa.close()
        if _original is None:
            raise _engine.Unsupported('contig names repeat in {}'.format(fasta))
        return _original(fasta, RE, keep_letter_case, logger)
    logger.info('Parsing input FASTA file...')
    return table


def _agp_lines(group, pieces, Ns, corrected_ctg_set):
    """write_agp :89-122 of one group: (lines of .agp, lines of .raw.agp)"""
    agp, raw = [], []
    n = acc = 0
    for ctg, ori, ctg_len in pieces:
        n += 1
        start, end = acc + 1, acc + ctg_len
        acc += ctg_len
        line = '{}\t{}\t{}\t{}\tW\t{}\t1\t{}\t{}\n'.format(group, start, end, n, ctg, ctg_len, ori)
        agp.append(line)
        if ctg in corrected_ctg_set:
            assert ':' in ctg
            raw_ctg, pos_range = ctg.rsplit(':', 1)
            s, e = pos_range.split('-')
            raw.append('{}\t{}\t{}\t{}\tW\t{}\t{}\t{}\t{}\n'.format(group, start, end, n, raw_ctg, s, e, ori))
        else:
            raw.append(line)
        if n < len(pieces) * 2 - 1:
            n += 1
            gap = '{}\t{}\t{}\t{}\tU\t{}\tscaffold\tyes\tproximity_ligation\n'.format(group, acc + 1, acc + Ns, n, Ns)
            acc += Ns
            agp.append(gap)
            raw.append(gap)
    return agp, raw


def build_final_scaffolds(tour_dict, fa_dict, output_ctgs, corrected_ctg_set, args, _original=None, _logger=logger):
    """build_final_scaffolds() :74-179 on a frozen FastaTable"""
    Ns, width = args.Ns, args.max_width
    if not (isinstance(fa_dict, FastaTable) and fa_dict.frozen) or width < 1 or Ns < 0:
        if _original is None:
            raise ValueError('build_final_scaffolds: not served here (a frozen FastaTable, max_width >= 1 and Ns >= 0 are)')
        return _original(tour_dict, fa_dict, output_ctgs, corrected_ctg_set, args)
    names, lengths = fa_dict.names, fa_dict.lengths
    groups = list(tour_dict)
    ids = [np.fromiter((fa_dict.index_of(ctg) for ctg, _ori in tour_dict[g]), np.int64, len(tour_dict[g])) for g in groups]
    if any((x < 0).any() for x in ids):                          # fa_dict[ctg] :137 raises KeyError
        if _original is None:
            raise KeyError('a contig of a tour is not in the FASTA file')
        return _original(tour_dict, fa_dict, output_ctgs, corrected_ctg_set, args)
    if not args.sort_by_input:                                   # :136-140: list.sort(reverse=True) is stable
        total = [int(lengths[x].sum()) + (len(x) - 1) * Ns for x in ids]      # (an empty tour: -Ns)
        order = sorted(range(len(groups)), key=lambda k: -total[k])
    else:
        order = range(len(groups))
    anchored = np.zeros(len(names), bool)
    for ctg in output_ctgs:
        k = fa_dict.index_of(ctg)
        if k >= 0:
            anchored[k] = True
    rest = np.flatnonzero(~anchored)
    rest = rest[np.argsort(-lengths[rest], kind='stable')]      # :150

    rec_names, piece_off, piece_ctg, piece_rev = [], [0], [], []
    agp, raw = [], []
    try:
        for k in order:
            g, pieces = groups[k], tour_dict[groups[k]]
            rec_names.append(g)
            piece_ctg.extend(ids[k].tolist())
            piece_rev.extend(ori != '+' for _ctg, ori in pieces)     # :80-83: everything but '+' is reversed
            piece_off.append(len(piece_ctg))
            a, r = _agp_lines(g, [(ctg, ori, int(lengths[i])) for (ctg, ori), i in zip(pieces, ids[k])], Ns, corrected_ctg_set)
            agp.extend(a)
            raw.extend(r)
        for i in rest.tolist():                                  # :164-179
            ctg, ctg_len = names[i], int(lengths[i])
            rec_names.append(ctg)
            piece_ctg.append(i)
            piece_rev.append(False)
            piece_off.append(len(piece_ctg))
            line = '{0}\t1\t{1}\t1\tW\t{0}\t1\t{1}\t+\n'.format(ctg, ctg_len)
            agp.append(line)
            if ctg in corrected_ctg_set:
                assert ':' in ctg
                raw_ctg, pos_range = ctg.rsplit(':', 1)
                start, end = pos_range.split('-')
                raw.append('{0}\t1\t{2}\t1\tW\t{1}\t{3}\t{4}\t+\n'.format(ctg, raw_ctg, ctg_len, start, end))
            else:
                raw.append(line)
    except (AssertionError, ValueError):
        if _original is None:
            raise
        return _original(tour_dict, fa_dict, output_ctgs, corrected_ctg_set, args)
    try:
        fa_dict.engine.emit('{}.fa'.format(args.prefix), rec_names, piece_off, piece_ctg, piece_rev, Ns, width)
    except fa_dict.engine.Unsupported:
        if _original is None:
            raise
        return _original(tour_dict, fa_dict, output_ctgs, corrected_ctg_set, args)
    _logger.info('Building final scaffolds...')
    with open('{}.agp'.format(args.prefix), 'w') as agp_out, open('{}.raw.agp'.format(args.prefix), 'w') as raw_agp_out:
        agp_out.write(''.join(agp))
        raw_agp_out.write(''.join(raw))
