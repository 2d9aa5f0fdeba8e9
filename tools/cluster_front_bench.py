#!/usr/bin/env python3
"""Measures the front of `haphic cluster` (run() :2785-2831: parse_fasta, parse_gfa, the bookkeeping of --correct_nrounds with the corrected_asm.fa
loop, stat_fragments) with the seams of patch_reference(H, front=True) against the parent's bound seams on the same files in the same session, and
writes profiles/cluster_front_bench.json.  A record, not a gate.

    python tools/cluster_front_bench.py [--contigs 100000] [--bases 3000000000] [--small-bases 30000000] [--repeats 3]      (one MI355X)

The assembly is the synthetic one of tools/reassign_front_bench.py (write_assembly); the GFA is hifiasm-shaped: one S line per contig with a sequence
of its length on the line, LN and rd tags, and --a-lines A lines behind them.  Yardsticks, all on the same files:
  * parse_fasta + stat_fragments: cluster.parse_fasta and cluster.stat_fragments on the plain rows it returns — what patch_reference(H) binds;
  * parse_gfa: the parent binds nothing, the reference's own per-line loop runs; it is restated here (host_parse_gfa) so that the tool runs where
    the reference is absent;
  * correction: correct.update_bookkeeping on plain rows, then the loop of correct_assembly :1267-1269 that writes corrected_asm.fa.
Repeats alternate seam and yardstick; every figure is reported as median, min and max, with the library's profiling off; the kernel times are its
HIP events in one more run that is not timed.  --rehearse runs every leg on the host stand-ins of tests/ without a device (tiny sizes; the figures
mean nothing)."""
import argparse
import json
import logging
import os
import statistics
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from reassign_front_bench import write_assembly      # noqa: E402

clock = time.perf_counter
KERNELS = ('fa_high', 'fa_breaks', 'fa_classify', 'fa_tables', 'fa_copy', 're_block_counts', 'gfa_count', 'gfa_starts', 'gfa_mark', 'gfa_fields', 'gfa_names')
STAT = dict(nchrs=24, flank=500, Nx=80, bin_size=-1)       # the defaults of `haphic cluster`
LOG = logging.getLogger('cluster_front_bench')
LOG.propagate = False
LOG.addHandler(logging.NullHandler())


def spread(values):
    return {'median_s': statistics.median(values), 'min_s': min(values), 'max_s': max(values), 'runs': len(values)}


def write_gfa(paths, n_ctg, n_bases, n_a_lines, seed=12):
    """contig k goes to file k % len(paths): 'S', name, a sequence of its length, LN:i:, rd:i:; then the file's share of the A lines"""
    rng = np.random.default_rng(seed)
    block = np.frombuffer(b'ACGT', np.uint8)[rng.integers(0, 4, 64 << 20, dtype=np.uint8)].tobytes()
    weights = rng.uniform(0.2, 1.8, n_ctg)
    lengths = np.minimum(np.maximum(1, (weights / weights.sum() * n_bases).astype(np.int64)), len(block) // 2)
    starts = rng.integers(0, len(block) // 2, n_ctg)
    a_block = b''.join(b'A\tctg%06d\t%d\t+\tm64011_%07d/ccs\t0\t15000\tid:i:%d\tHG:A:a\n' % (k % n_ctg, 1000 * k, k, k) for k in range(1000))
    files = [open(p, 'wb', buffering=8 << 20) for p in paths]
    view = memoryview(block)
    for k, (L, s) in enumerate(zip(lengths.tolist(), starts.tolist())):
        f = files[k % len(files)]
        f.write(b'S\tctg%06d\t' % k)
        f.write(view[s:s + L])
        f.write(b'\tLN:i:%d\trd:i:%d\n' % (L, 20 + k % 17))
    for f in files:
        for _ in range(n_a_lines // 1000 // len(files)):
            f.write(a_block)
        f.close()
    return lengths


def host_parse_gfa(paths):
    """the per-line host loop over the GFA files (what runs with parse_gfa unbound): every line passes through Python, the S lines are split"""
    out = {}
    for n, path in enumerate(paths):
        with open(path) as f:
            for line in f:
                if line[:2] == 'S\t':
                    cols = line.split('\t')
                    out[cols[1]] = (n, int(cols[4].rsplit(':', 1)[-1]), int(cols[3].rsplit(':', 1)[-1]))
    return out


def modules(rehearse):
    """(the module with the front bound, the module as patch_reference(H) leaves it)"""
    from haphic_amd import assembly, cluster
    engines = (None, None)
    if rehearse:
        from tests import assembly_cases, oracle_lib
        cluster._lib = oracle_lib
        engines = (assembly_cases.fasta_engine(), assembly_cases.HostGfa)
    parent = types.SimpleNamespace(parse_fasta=cluster.parse_fasta, stat_fragments=cluster.stat_fragments, logger=LOG,
                                   parse_gfa=lambda gfa_list, fa_dict, logger=LOG: host_parse_gfa(gfa_list))
    front = types.SimpleNamespace(stat_fragments=cluster.stat_fragments, logger=LOG)
    front.parse_fasta = assembly.bind_fasta(parent, engines[0], original=cluster.parse_fasta)
    front.parse_gfa = assembly.bind_gfa(parent, engines[1])
    return front, parent


def time_front(M, fasta):
    t0 = clock()
    fa_dict = M.parse_fasta(fasta, RE='GATC', logger=LOG)
    t1 = clock()
    out = M.stat_fragments(fa_dict, 'GATC', {}, set(), logger=LOG, **STAT)
    t2 = clock()
    return {'parse_fasta_s': t1 - t0, 'stat_fragments_s': t2 - t1, 's': t2 - t0}, (out[2], out[3], out[5], [(n, v[1], v[2]) for n, v in fa_dict.items()])


def leg_front(front, parent, fasta, repeats, label):
    time_front(front, fasta)                                                            # warm
    ours, theirs, same = [], [], None
    for r in range(repeats):
        got, a = time_front(front, fasta)
        want, b = time_front(parent, fasta)
        ours.append(got)
        theirs.append(want)
        same = a == b
        del a, b
        print(label, r, json.dumps({'seam': got, 'yardstick': want}), flush=True)
    assert same, 'the seam and the yardstick disagree'
    return {who: {k: spread([x[k] for x in runs]) for k in ('parse_fasta_s', 'stat_fragments_s', 's')} for who, runs in (('seam', ours), ('yardstick', theirs))}


def leg_gfa(front, parent, paths, fa_dict, repeats, label):
    ours, theirs = [], []
    front.parse_gfa(paths, fa_dict, logger=LOG)                                         # warm
    for r in range(repeats):
        t0 = clock()
        got = front.parse_gfa(paths, fa_dict, logger=LOG)
        t1 = clock()
        want = parent.parse_gfa(paths, fa_dict)
        t2 = clock()
        ours.append(t1 - t0)
        theirs.append(t2 - t1)
        assert list(got.items()) == [(k, v[:2]) for k, v in want.items()] and len(got) == len(fa_dict), 'the seam and the yardstick disagree'
        print(label, r, json.dumps({'seam_s': t1 - t0, 'yardstick_s': t2 - t1}), flush=True)
    return {'seam': spread(ours), 'yardstick': spread(theirs), 'file_bytes': sum(os.path.getsize(p) for p in paths), 'records': len(fa_dict)}


def leg_correction(front, parent, fasta, out_path, repeats, every):
    """one round that breaks every `every`-th contig in three, then the loop that writes corrected_asm.fa; rows as the parent has them, rows with
    per-row fetch, rows with one bulk fetch"""
    from haphic_amd import assembly, correct
    args = types.SimpleNamespace(RE='GATC')

    def run(fa_dict):
        names = [n for k, n in enumerate(fa_dict) if k % every == 0 and fa_dict[n][1] > 100]
        points = {n: [(fa_dict[n][1] // 3, 3), (2 * (fa_dict[n][1] // 3), 3)] for n in names}
        src, fpos, ffrag = {n: n for n in names}, {n: [0] for n in names}, {n: [n] for n in names}
        t0 = clock()
        correct.update_bookkeeping(points, src, fpos, ffrag, fa_dict, {}, set(fa_dict), args)
        t1 = clock()
        with open(out_path, 'w') as f:
            for ctg, ctg_info in fa_dict.items():
                f.write('>{}\n{}\n'.format(ctg, ctg_info[0]))
        t2 = clock()
        stat = front.stat_fragments(fa_dict, 'GATC', {}, set(), logger=LOG, **STAT)
        t3 = clock()
        return {'bookkeeping_s': t1 - t0, 'write_s': t2 - t1, 'stat_fragments_s': t3 - t2, 's': t3 - t0}, (os.path.getsize(out_path), stat[5], len(names))
    plain = parent.parse_fasta(fasta, RE='GATC', logger=LOG)
    runs, check = {'yardstick': [], 'per_row': [], 'bulk': []}, {}
    for r in range(repeats):
        for who in ('bulk', 'yardstick', 'per_row'):
            if who == 'yardstick':
                fa_dict = {n: list(v) for n, v in plain.items()}
            else:
                assembly.BULK_FETCH = who == 'bulk'
                fa_dict = front.parse_fasta(fasta, RE='GATC', logger=LOG)
            got, check[who] = run(fa_dict)
            runs[who].append(got)
            del fa_dict
            print('correction', who, r, json.dumps(got), flush=True)
    assert check['bulk'] == check['yardstick'] == check['per_row'], 'the fetch forms and the yardstick disagree'
    os.remove(out_path)
    out = {who: {k: spread([x[k] for x in v]) for k in ('bookkeeping_s', 'write_s', 'stat_fragments_s', 's')} for who, v in runs.items()}
    out['broken_contigs'], out['file_bytes'] = check['bulk'][2], check['bulk'][0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--contigs', type=int, default=100000)
    ap.add_argument('--bases', type=int, default=3_000_000_000)
    ap.add_argument('--small-contigs', type=int, default=1000)
    ap.add_argument('--small-bases', type=int, default=30_000_000)
    ap.add_argument('--a-lines', type=int, default=2_000_000)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--break-every', type=int, default=50)
    ap.add_argument('--dir', default=None, help='where the files are written (default: a temporary directory)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cluster_front_bench.json'))
    ap.add_argument('--files-only', action='store_true', help='write the files and stop (a rehearsal without a device)')
    ap.add_argument('--rehearse', action='store_true', help='every leg on the host stand-ins of tests/ (no device; the figures mean nothing)')
    args = ap.parse_args()
    record = {'contigs': args.contigs, 'repeats': args.repeats, 'stat_fragments': STAT, 'rehearsal': args.rehearse,
              'yardstick': {'front': 'cluster.parse_fasta + cluster.stat_fragments on plain rows (what patch_reference(H) binds)',
                            'gfa': 'the per-line host loop (parse_gfa is unbound in the parent), restated in this tool',
                            'correction': 'correct.update_bookkeeping on plain rows + the loop of correct_assembly :1267-1269'}}
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        fasta, small = os.path.join(tmp, 'asm.fa'), os.path.join(tmp, 'small.fa')
        t0 = clock()
        bases = write_assembly(fasta, args.contigs, args.bases)[0]
        small_bases = write_assembly(small, args.small_contigs, args.small_bases, seed=13)[0]
        gfa1 = [os.path.join(tmp, 'asm.gfa')]
        gfa4 = [os.path.join(tmp, 'hap%d.gfa' % k) for k in range(4)]
        write_gfa(gfa1, args.contigs, args.bases, args.a_lines)
        record['files'] = {'bases': bases, 'fasta_bytes': os.path.getsize(fasta), 'small_bases': small_bases, 'small_fasta_bytes': os.path.getsize(small),
                           'gfa_bytes': os.path.getsize(gfa1[0]), 'a_lines': args.a_lines, 'write_s': clock() - t0}
        print('files', json.dumps(record['files']), flush=True)
        if args.files_only:
            return
        from haphic_amd import _lib
        front, parent = modules(args.rehearse)
        record['front_small'] = leg_front(front, parent, small, args.repeats, 'front_small')
        record['front'] = leg_front(front, parent, fasta, args.repeats, 'front')
        lengths = {('ctg%06d' % k): [None, 0, 1] for k in range(args.contigs)}
        for name, v in host_parse_gfa(gfa1).items():
            lengths[name][1] = v[2]
        record['gfa_one_file'] = leg_gfa(front, parent, gfa1, lengths, args.repeats, 'gfa_one_file')
        os.remove(gfa1[0])
        write_gfa(gfa4, args.contigs, args.bases, args.a_lines)
        record['gfa_four_files'] = leg_gfa(front, parent, gfa4, lengths, args.repeats, 'gfa_four_files')
        if not args.rehearse:                                                           # one more run, not timed: the events slow the host
            _lib.profile_enable(True)
            _lib.profile_reset()
            front.parse_gfa(gfa4, lengths, logger=LOG)
            time_front(front, fasta)
            record['kernel_ms'] = {k: _lib.profile_get(k)[0] for k in KERNELS}
            _lib.profile_enable(False)
        for p in gfa4:
            os.remove(p)
        record['correction'] = leg_correction(front, parent, fasta, os.path.join(tmp, 'corrected_asm.fa'), max(1, args.repeats - 1), args.break_every)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1, sort_keys=True)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
