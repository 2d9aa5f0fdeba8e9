#!/usr/bin/env python3
"""Measures `haphic refsort` on the device (haphic_amd/refsort.py: csrc/hhx_paf.hip, hhx_lis_sums, hhx_fasta_emit_segments) on a synthetic assembly and
writes profiles/refsort_bench.json.  A record, not a gate.

    python tools/refsort_bench.py [--mb 3000 30] [--dir /dev/shm] [--out profiles/refsort_bench.json]
    python tools/refsort_bench.py --reference-only --reference path/to/HapHiC/scripts [--mb 30] [--prefix-lines 100000]     (no GPU)

The assembly: contigs of 100 kb in ~24 groups (scaffolds.agp as `haphic build` writes it: random orientations, gaps of 100 N) and a twentieth of them
unanchored; the PAF file: 33 alignments of 6 kb per contig placed along the group's chromosome, half of the groups reversed against it, a fiftieth of the
lines with mapq 0 or on another chromosome — about 10^6 lines at 3 Gb — in two dialects: bare (12 fields) and with a cg:Z: tail of 2 to 4 kB.
Timed, medians of three alternating repeats with min and max, profiling off: parse_paf on both dialects, the LIS step (flattening + hhx_lis_sums; one
more untimed run with profiling on gives the kernel's HIP-event time), order_and_orient_groups to the complete scaffolds.refsort.fa, the three
together as run() :398-409 calls them, and plainly writing the same output bytes to the same directory — the floor of the FASTA step.
Yardstick: the reference's own functions on the same generator where its checkout is given (--reference-only, no GPU needed); elsewhere that
record is carried over from the existing file, labelled `stored: true`.  Where the reference cannot finish a size in minutes it runs a prefix of
the groups and the figure is marked `extrapolated` with how.  The reference is timed three times where a size takes seconds, once where it takes
minutes.  The device side needs no checkout: parse_agp and the alignment check around the seams are the restatements of tests/refsort_cases.py, and
the reference module is loaded by tests/golden/make_golden_refsort.py's loader; the record says so.  The default rule (verdict()) sets the slowest
device repeat against the fastest reference run, names a yardstick stored from another box and then asks for a factor of 2."""
import argparse
import contextlib
import io
import json
import os
import platform
import statistics
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONTIG, COLUMNS, N_GROUPS, ALN_PER_CTG, ALN_LEN, ALN_STEP, GAP = 100_000, 60, 24, 33, 6000, 2900, 100


def synth(directory, n_mb, seed=4):
    """asm.fa of about n_mb MB, scaffolds.agp, bare.paf and tails.paf -> dict of paths and counts"""
    rng = np.random.default_rng(seed)
    n_ctg = max(int(n_mb * 1e6) // CONTIG, 2 * N_GROUPS)
    pool = np.frombuffer(b'ACGT', np.uint8)[rng.integers(0, 4, 1 << 24)]
    pool = np.where(rng.random(1 << 24) < 0.1, pool | 0x20, pool).astype(np.uint8)
    rows = -(-CONTIG // COLUMNS)
    tail = CONTIG - (rows - 1) * COLUMNS
    fasta = os.path.join(directory, 'asm.fa')
    with open(fasta, 'wb') as f:
        for k in range(n_ctg):
            at = int(rng.integers(0, pool.size - CONTIG))
            body = np.full((rows, COLUMNS + 1), ord('\n'), np.uint8)
            body[:rows - 1, :COLUMNS] = pool[at:at + (rows - 1) * COLUMNS].reshape(rows - 1, COLUMNS)
            body[rows - 1, :tail] = pool[at + (rows - 1) * COLUMNS:at + CONTIG]
            f.write(b'>ctg%06d length=%d\n' % (k, CONTIG))
            f.write(body.tobytes()[:(rows - 1) * (COLUMNS + 1) + tail + 1])
    order = rng.permutation(n_ctg)
    anchored, loose = order[:n_ctg * 19 // 20], order[n_ctg * 19 // 20:]
    cigar = ''.join('%d%s' % (n, 'MIDM'[k % 4]) for k, n in enumerate(rng.integers(1, 400, 2000)))
    paths = {'fasta': fasta, 'agp': os.path.join(directory, 'scaffolds.agp'), 'bare': os.path.join(directory, 'bare.paf'),
             'tails': os.path.join(directory, 'tails.paf')}
    files = {key: open(paths[key], 'w') for key in ('agp', 'bare', 'tails')}
    n_lines = 0
    for g, part in enumerate(np.array_split(anchored, N_GROUPS)):
        agp, bare, tails = [], [], []
        group, chrom, acc = 'group%d' % (g + 1), 'chr%02d' % (g + 1), 0
        total = part.size * CONTIG + (part.size - 1) * GAP
        flipped = g % 2 == 1                                     # the group lies reversed on its chromosome
        for n, (k, o) in enumerate(zip(part.tolist(), rng.integers(0, 2, part.size).tolist())):
            if n:
                agp.append('%s\t%d\t%d\t%d\tU\t%d\tscaffold\tyes\tproximity_ligation\n' % (group, acc + 1, acc + GAP, 2 * n, GAP))
                acc += GAP
            agp.append('%s\t%d\t%d\t%d\tW\tctg%06d\t1\t%d\t%s\n' % (group, acc + 1, acc + CONTIG, 2 * n + 1, k, CONTIG, '+-'[o]))
            noise = rng.random(ALN_PER_CTG)
            for i in range(ALN_PER_CTG):
                qs = i * ALN_STEP
                qe = qs + ALN_LEN
                pos = acc + (qs if o == 0 else CONTIG - qe)      # where the alignment lies in the group
                rs = total - pos - ALN_LEN if flipped else pos
                strand = '+-'[o ^ flipped]
                mapq, ref = 60, chrom
                if noise[i] < 0.01:
                    mapq = 0
                elif noise[i] < 0.02:
                    ref = 'chr%02d' % ((g + 7) % N_GROUPS + 1)
                line = 'ctg%06d\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d' % (k, CONTIG, qs, qe, strand, ref, 200_000_000, rs, rs + ALN_LEN, ALN_LEN - 40, ALN_LEN, mapq)
                bare.append(line + '\n')
                cut = int(noise[i] * 2000)
                tails.append(line + '\tNM:i:40\tms:i:5800\ttp:A:P\tcg:Z:' + cigar[cut:cut + 2000 + cut] + '\n')
                n_lines += 1
            acc += CONTIG
        for key, lines in (('agp', agp), ('bare', bare), ('tails', tails)):
            files[key].write(''.join(lines))
    for k in loose.tolist():
        files['agp'].write('ctg%06d\t1\t%d\t1\tW\tctg%06d\t1\t%d\t+\n' % (k, CONTIG, k, CONTIG))
    for f in files.values():
        f.close()
    return dict(paths, contigs=n_ctg, paf_lines=n_lines, fasta_bytes=os.path.getsize(fasta), bare_bytes=os.path.getsize(paths['bare']),
                tails_bytes=os.path.getsize(paths['tails']))


def args_for(s, paf, fout='scaffolds.refsort.fa'):
    return types.SimpleNamespace(agp=s['agp'], paf=s[paf], fasta=s['fasta'], min_ctg_len=10, aln_len_cutoff=5000, skip_aln_check=False, keep_original_ids=False,
                                 max_width=COLUMNS, fout=fout, ref_order=None)


def box():
    return '{}, {} CPUs'.format(platform.machine(), os.cpu_count())


def in_dir(directory, fn):
    cwd = os.getcwd()
    os.chdir(directory)
    try:
        return fn()
    finally:
        os.chdir(cwd)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def summary(seconds):
    return {'seconds': round(statistics.median(seconds), 4), 'min': round(min(seconds), 4), 'max': round(max(seconds), 4), 'repeats': len(seconds)}


def quiet(fn):
    with contextlib.redirect_stdout(io.StringIO()) as out:
        res = fn()
    return res, len(out.getvalue())


def reference_record(scripts, n_mb, directory, prefix_lines):
    """the reference's own functions, one core.  parse_paf on the tails dialect and find_lis run on a prefix where the whole would take minutes"""
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    from make_golden_refsort import load_reference_refsort
    F = load_reference_refsort(scripts)
    F.logger.setLevel('ERROR')
    rec = {'what': 'HapHiC_refsort parse_paf, order_and_orient_groups and HapHiC_cluster.parse_fasta on the same generator, one core', 'stored': False, 'box': box()}
    with tempfile.TemporaryDirectory(dir=directory) as tmp:
        s = synth(tmp, n_mb)
        rec.update(mb=n_mb, contigs=s['contigs'], paf_lines=s['paf_lines'], fasta_bytes=s['fasta_bytes'], bare_bytes=s['bare_bytes'], tails_bytes=s['tails_bytes'])
        args = args_for(s, 'bare')
        ctg_group, group_lines, group_len, solo = F.parse_agp(args.agp, args.min_ctg_len)
        t_bare, group_ref = timed(lambda: F.parse_paf(s['bare'], ctg_group, args.aln_len_cutoff))
        rec['parse_paf_bare_seconds'] = round(t_bare, 3)
        n = min(prefix_lines, s['paf_lines'])
        head = os.path.join(tmp, 'head.paf')
        with open(s['tails']) as f, open(head, 'w') as g:
            for _ in range(n):
                g.write(f.readline())
        t_head, _ = timed(lambda: F.parse_paf(head, ctg_group, args.aln_len_cutoff))
        rec['parse_paf_tails_seconds'] = round(t_head * s['paf_lines'] / n, 3)
        if n < s['paf_lines']:
            rec['parse_paf_tails_extrapolated'] = 'the first {} of {} lines took {:.3f} s; scaled by the line count (the loop is linear in the lines)'.format(n, s['paf_lines'], t_head)
        t_fa, fa_dict = timed(lambda: F.parse_fasta(s['fasta']))
        rec['parse_fasta_seconds'] = round(t_fa, 3)
        # order_and_orient_groups is O(n^2) per group in find_lis: time it whole on groups cut down to `per_group` alignments, and the largest group alone
        sizes = {g: len(max(r.values(), key=lambda x: x[1])[0]) for g, r in group_ref.items()}
        rec['alignments_per_group'] = {'min': min(sizes.values()), 'max': max(sizes.values())}
        per_group = 2000
        cut = {g: {ref: [v[0][:per_group], sum(a[1] for a in v[0][:per_group])] for ref, v in r.items()} for g, r in group_ref.items()}
        with open(os.path.join(tmp, 'ref.fa'), 'w') as fout:
            (t_cut, _), _n = quiet(lambda: timed(lambda: F.order_and_orient_groups(ctg_group, cut, group_lines, group_len, solo, args, fa_dict, fout)))
        (t_cut_nofa, _), _n = quiet(lambda: timed(lambda: F.order_and_orient_groups(ctg_group, cut, group_lines, group_len, solo, args)))
        rec['order_and_orient_groups_cut_seconds'] = round(t_cut, 3)
        rec['fasta_output_seconds'] = round(t_cut - t_cut_nofa, 3)
        rec['lis_cut_seconds'] = round(t_cut_nofa, 3)
        worst = max(sizes.values())
        scale = sum(min(n_, 10 ** 9) ** 2 for n_ in sizes.values()) / sum(min(n_, per_group) ** 2 for n_ in sizes.values())
        rec['lis_seconds'] = round(t_cut_nofa * scale, 3)
        if worst > per_group:
            rec['lis_extrapolated'] = ('every group cut to its first {} alignments took {:.3f} s without --fasta; scaled by the sum of n^2 over the groups '
                                       '(find_lis :199-204 is two nested loops over the group), x {:.1f}'.format(per_group, t_cut_nofa, scale))
        rec['run_seconds'] = round(t_bare + t_fa + rec['lis_seconds'] + rec['fasta_output_seconds'], 3)
        rec['run_note'] = 'parse_paf (bare) + parse_fasta + LIS (as above) + FASTA output; parse_agp and the check are the same code on both sides'
    return rec


def device_record(n_mb, directory):
    from haphic_amd import _lib, refsort, scaffolds
    from tests import refsort_cases as rc
    rec = {'mb': n_mb, 'box': box(), 'directory': directory,
               'note': 'parse_agp and alignment_check around the seams are the restatements of tests/refsort_cases.py (the reference checkout need not be on the '
                       'device box); `lis` is the flattening plus the hhx_lis_sums call, `lis_call` the call alone (host ranking + kernel), hip_events_ms.lis_sums '
                       'the kernel alone'}
    log = rc.ListLogger()
    with tempfile.TemporaryDirectory(dir=directory) as tmp:
        s = synth(tmp, n_mb)
        rec.update(contigs=s['contigs'], paf_lines=s['paf_lines'], fasta_bytes=s['fasta_bytes'], bare_bytes=s['bare_bytes'], tails_bytes=s['tails_bytes'])
        args = args_for(s, 'bare', os.path.join(tmp, 'scaffolds.refsort.fa'))
        _lib.Fasta(b'>a\nACGT\n').close()                          # the device and the library are up
        ctg_group, group_lines, group_len, solo = rc.parse_agp(args.agp, args.min_ctg_len)
        t = {k: [] for k in ('parse_paf_bare', 'parse_paf_tails', 'parse_fasta', 'lis', 'lis_call', 'order_and_orient_groups', 'order_and_orient_groups_no_fasta', 'run',
                             'plain_write')}
        fa_dict = None
        for _ in range(3):                                       # alternating: one of each per round
            dt, group_ref = timed(lambda: refsort.parse_paf(s['bare'], ctg_group, args.aln_len_cutoff, _logger=log))
            t['parse_paf_bare'].append(dt)
            dt, with_tails = timed(lambda: refsort.parse_paf(s['tails'], ctg_group, args.aln_len_cutoff, _logger=log))
            t['parse_paf_tails'].append(dt)
            assert with_tails == group_ref
            if fa_dict is not None:
                fa_dict.engine.close()
            dt, fa_dict = timed(lambda: scaffolds.parse_fasta(s['fasta'], logger=log))
            t['parse_fasta'].append(dt)

            def lis():
                groups, refs, ptr, value, weight = refsort._sequences(ctg_group, group_ref)
                t0 = time.perf_counter()
                sums = _lib.lis_sums(ptr, value, weight)
                return time.perf_counter() - t0, ptr, sums
            dt, (dt_call, ptr, sums) = timed(lis)
            t['lis'].append(dt)
            t['lis_call'].append(dt_call)
            with open(args.fout, 'w') as fout:
                (dt, _), n_stdout = quiet(lambda: timed(lambda: refsort.order_and_orient_groups(ctg_group, group_ref, group_lines, group_len, solo, args, fa_dict, fout,
                                                                                               _logger=log)))
            t['order_and_orient_groups'].append(dt)
            (dt, _), _n = quiet(lambda: timed(lambda: refsort.order_and_orient_groups(ctg_group, group_ref, group_lines, group_len, solo, args, _logger=log)))
            t['order_and_orient_groups_no_fasta'].append(dt)
            assert refsort.STATS == {'parse_paf': 'device', 'order_and_orient_groups': 'device'}, refsort.STATS

            def run():                                           # run() :398-409 around the three seams
                cg, gl, glen, so = rc.parse_agp(args.agp, args.min_ctg_len)
                gr = refsort.parse_paf(s['bare'], cg, args.aln_len_cutoff, _logger=log)
                rc.alignment_check(glen, gr, so, args.aln_len_cutoff)
                fa = scaffolds.parse_fasta(s['fasta'], logger=log)
                with open(args.fout, 'w') as fout:
                    refsort.order_and_orient_groups(cg, gr, gl, glen, so, args, fa, fout, _logger=log)
                fa.engine.close()
            (dt, _), _n = quiet(lambda: timed(run))
            t['run'].append(dt)
            data = open(args.fout, 'rb').read()

            def plain():
                with open(os.path.join(tmp, 'plain.fa'), 'wb') as f:
                    f.write(data)
            t['plain_write'].append(timed(plain)[0])
        rec['scaffolds_refsort_fa_bytes'] = len(data)
        rec['stdout_bytes'] = n_stdout
        del data
        sizes = np.diff(ptr)
        rec['lis_sequences'] = {'groups': int(sizes.size), 'min': int(sizes.min()), 'max': int(sizes.max()), 'elements': int(sizes.sum())}
        rec['lis_sums_forward_reverse'] = [[int(a), int(b)] for a, b in zip(*sums)][:4]
        for k, v in t.items():
            rec[k] = summary(v)
        rec['fasta_output'] = summary([a - b for a, b in zip(t['order_and_orient_groups'], t['order_and_orient_groups_no_fasta'])])
        rec['fasta_output_over_plain_write'] = round(rec['fasta_output']['seconds'] / rec['plain_write']['seconds'], 2)
        _lib.profile_enable(True)                                # one more run, untimed, for the HIP-event times
        _lib.profile_reset()
        refsort.parse_paf(s['tails'], ctg_group, args.aln_len_cutoff, _logger=log)
        with open(args.fout, 'w') as fout:
            quiet(lambda: refsort.order_and_orient_groups(ctg_group, group_ref, group_lines, group_len, solo, args, fa_dict, fout, _logger=log))
        rec['hip_events_ms'] = {}
        for k in ('paf_count', 'paf_starts', 'paf_lines', 'paf_fields', 'paf_names', 'lis_sums', 'fa_emit'):
            ms, launches = _lib.profile_get(k)
            rec['hip_events_ms'][k] = {'ms': round(ms, 3), 'launches': launches}
        _lib.profile_enable(False)
        fa_dict.engine.close()
    return rec


def combine(runs):
    """the repeats of one size of the reference: every *_seconds figure becomes the median, with the spread beside it"""
    out = dict(runs[0], repeats=len(runs))
    out['spread'] = {}
    for k in [k for k in runs[0] if k.endswith('_seconds')]:
        v = [r[k] for r in runs]
        out[k] = round(statistics.median(v), 3)
        out['spread'][k] = [min(v), max(v)]
    return out


def verdict(device, reference):
    """the default rule: a seam is bound by default only if no measured size loses to the reference beyond the spread of the repeats: the SLOWEST
    device repeat against the FASTEST run of the reference.  A yardstick carried over from another box (`stored`) is named as such: the
    reference is Python on one core, so the other box's core enters every figure, and a piece counts as won only by a factor of 2 or more then"""
    out, notes = {}, []
    ref = {r['mb']: r for r in reference}
    for d in device:
        r = ref.get(d['mb'])
        if r is None:
            continue
        low = lambda k: min(r.get('spread', {}).get(k, [r[k]]))      # noqa: E731
        margin = 2.0 if r.get('stored') else 1.0
        if r.get('stored'):
            notes.append('{} Mb: the reference figures are stored from another box ({}; {} run(s) per figure): a piece wins only by a factor of 2'.format(
                d['mb'], r['box'], r.get('repeats', 1)))
        for k in (x for x in r if x.endswith('_extrapolated')):
            notes.append('{} Mb: {}: {}'.format(d['mb'], k, r[k]))
        out[str(d['mb'])] = {piece: {'device_max': ours, 'reference_min': theirs, 'wins': ours * margin <= theirs} for piece, ours, theirs in (
            ('parse_paf_bare', d['parse_paf_bare']['max'], low('parse_paf_bare_seconds')), ('parse_paf_tails', d['parse_paf_tails']['max'], low('parse_paf_tails_seconds')),
            ('parse_fasta', d['parse_fasta']['max'], low('parse_fasta_seconds')),
            ('lis', d['order_and_orient_groups_no_fasta']['max'], low('lis_seconds')), ('fasta_output', d['fasta_output']['max'], low('fasta_output_seconds')),
            ('run', d['run']['max'], low('run_seconds')))}
    loses = sorted({k for v in out.values() for k, c in v.items() if not c['wins']})
    return {'seconds': out, 'loses': loses, 'yardstick': notes,
            'default': 'bound' if out and not loses else ('opt-in: ' + ', '.join(loses) if loses else 'not decided: no size has both sides')}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mb', type=float, nargs='+', default=[3000, 30])
    ap.add_argument('--dir', default='/dev/shm' if os.path.isdir('/dev/shm') else None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'refsort_bench.json'))
    ap.add_argument('--reference', default=os.environ.get('HAPHIC_REFERENCE'))
    ap.add_argument('--reference-only', action='store_true')
    ap.add_argument('--prefix-lines', type=int, default=100000)
    a = ap.parse_args()
    old = json.load(open(a.out)) if os.path.exists(a.out) else {}
    rec = {'what': 'haphic refsort on the device against the reference\'s own functions on the same generator (tools/refsort_bench.py)',
           'device': old.get('device', []), 'reference': old.get('reference', [])}
    if a.reference_only:
        scripts = a.reference if os.path.isfile(os.path.join(a.reference or '', 'HapHiC_refsort.py')) else os.path.join(a.reference, 'scripts')
        new = [combine([reference_record(scripts, mb, a.dir, a.prefix_lines) for _ in range(3 if mb <= 300 else 1)]) for mb in a.mb]
        rec['reference'] = new + [r for r in rec['reference'] if r['mb'] not in a.mb]
    else:
        new = [device_record(mb, a.dir) for mb in a.mb]
        rec['device'] = new + [r for r in rec['device'] if r['mb'] not in a.mb]
        for r in rec['reference']:
            r['stored'] = True
    rec['default_rule'] = verdict(rec['device'], rec['reference'])
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps(new)[:3000])


if __name__ == '__main__':
    main()
