#!/usr/bin/env python3
"""Measures "File parsing and data preparation" of `haphic reassign` (run() :782-858: parse_fasta, parse_pickle, parse_link_dict) with the seams of
patch_reassign(R, rounds=True, pickle=True, resident=True, fasta=True) against the parent's paths on the same files in the same session, and
writes profiles/reassign_front_bench.json.  A record, not a gate.

    python tools/reassign_front_bench.py [--contigs 100000] [--bases 3000000000] [--keys 5000000,115000000] [--repeats 3]      (one MI355X)

The assembly is synthetic (--contigs contigs, --bases bases in lines of 60, lengths spread 1 : 9), the tables are the synthetic ones of
tools/reassign_bench.py under the same contig names.  Yardsticks:
  * FASTA: cluster.parse_fasta, this repository's restatement of the reference's per-line loop.  It is timed on the first --yardstick-bases bases
    of the same assembly and scaled by the bases ("extrapolated": the loop is linear in the lines; at full size it holds the genome three times
    over as Python strings, and three repeats of it would take most of a session) unless --yardstick-bases covers the assembly;
  * tables: parse_pickle + parse_link_dict through patch_reassign(R, rounds=True, pickle=True), i.e. resident=False.
Every figure is the median of --repeats runs, with their spread (min, max), alternating seam and yardstick, with the library's profiling off;
kernel times are its HIP events in one more run that is not timed."""
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
clock = time.perf_counter
FASTA_KERNELS = ('fa_h2d', 'fa_high', 'fa_breaks', 'fa_classify', 'fa_tables', 'fa_copy', 're_block_counts')
TABLE_KERNELS = ('pkl_boundaries', 'pkl_walk', 'pkl_names', 'pkl_keys', 'reassign_check', 'groupstats_adjacency')
WIDTH = 60


def write_assembly(path, n_ctg, n_bases, seed=11, prefix_path=None, prefix_bases=0):
    """a FASTA of n_ctg contigs 'ctg%06d' and about n_bases bases in lines of WIDTH; the first contigs up to prefix_bases also go to prefix_path.
    -> (bases written, contigs in the prefix, bases in the prefix)"""
    rng = np.random.default_rng(seed)
    block_lines = (32 << 20) // WIDTH
    block = np.empty((block_lines, WIDTH + 1), np.uint8)
    block[:, :WIDTH] = np.frombuffer(b'ACGT', np.uint8)[rng.integers(0, 4, (block_lines, WIDTH))]
    block[:, WIDTH] = ord('\n')
    flat = memoryview(block.reshape(-1))
    weights = rng.uniform(0.2, 1.8, n_ctg)
    lengths = np.maximum(1, (weights / weights.sum() * n_bases).astype(np.int64))
    lengths = np.minimum(lengths, (block_lines - 1) * WIDTH)
    starts = rng.integers(0, block_lines, n_ctg)
    total = in_prefix = prefix_ctgs = 0
    with open(path, 'wb', buffering=8 << 20) as f:
        pf = open(prefix_path, 'wb', buffering=8 << 20) if prefix_path else None
        for k, (L, s) in enumerate(zip(lengths.tolist(), starts.tolist())):
            lines, rest = divmod(L, WIDTH)
            s = min(s, block_lines - lines - 1)
            a = s * (WIDTH + 1)
            body = flat[a:a + lines * (WIDTH + 1) + rest]
            head = b'>ctg%06d len=%d\n' % (k, L)
            tail = b'\n' if rest else b''
            for out in (f, pf if pf is not None and in_prefix < prefix_bases else None):
                if out is not None:
                    out.write(head)
                    out.write(body)
                    out.write(tail)
            if pf is not None and in_prefix < prefix_bases:
                in_prefix += L
                prefix_ctgs += 1
            total += L
        if pf is not None:
            pf.close()
    return total, prefix_ctgs, in_prefix


def stand_in(resident, fasta):
    from haphic_amd import cluster, patch
    R = types.ModuleType('HapHiC_reassign_stand_in')
    R.logger = logging.getLogger('reassign_front_bench')
    R.parse_fasta = cluster.parse_fasta
    for name in ('parse_pickle', 'parse_link_dict', 'run_reassignment', 'agglomerative_hierarchical_clustering', 'split_clm_file'):
        setattr(R, name, None)
    patch.patch_reassign(R, rounds=True, pickle=True, resident=resident, fasta=fasta)
    return R


def spread(values):
    return {'median_s': statistics.median(values), 'min_s': min(values), 'max_s': max(values), 'runs': len(values)}


def kernel_ms(names):
    from haphic_amd import _lib
    out = {k: _lib.profile_get(k)[0] for k in names}
    out['total'] = sum(out.values())
    return out


def time_fasta(R, path, profile=False):
    from haphic_amd import _lib
    if profile:
        _lib.profile_enable(True)
        _lib.profile_reset()
    t0 = clock()
    fa_dict = R.parse_fasta(path, RE='GATC', logger=R.logger)
    dt = clock() - t0
    out = {'s': dt, 'contigs': len(fa_dict), 'bases': sum(info[1] for info in fa_dict.values()), 're_sites': sum(info[2] - 1 for info in fa_dict.values())}
    if profile:
        out['kernel_ms'] = kernel_ms(FASTA_KERNELS)
        _lib.profile_enable(False)
    return out, fa_dict


def time_tables(R, path, fa_dict, ctg_group_dict, profile=False):
    from haphic_amd import _lib
    if profile:
        _lib.profile_enable(True)
        _lib.profile_reset()
    t0 = clock()
    link_dict, _sorted, _re = R.parse_pickle(fa_dict, path)
    t1 = clock()
    tables = R.parse_link_dict(link_dict, ctg_group_dict)
    t2 = clock()
    session = getattr(link_dict, '_session', None)
    out = {'parse_pickle_s': t1 - t0, 'parse_link_dict_s': t2 - t1, 's': t2 - t0, 'tables': type(tables[0]).__name__,
           'key_fetches': getattr(session, 'fetches', None), 'cells_checksum': int(tables[0]._job.engine.cells()[0].sum())}
    if profile:
        out['kernel_ms'] = kernel_ms(TABLE_KERNELS)
        _lib.profile_enable(False)
    tables[0]._job.engine.close()
    handle = getattr(session, 'handle', None)
    if handle is not None:
        handle.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--contigs', type=int, default=100000)
    ap.add_argument('--bases', type=int, default=3_000_000_000)
    ap.add_argument('--groups', type=int, default=32)
    ap.add_argument('--keys', default='5000000,115000000')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--yardstick-bases', type=int, default=300_000_000)
    ap.add_argument('--dir', default=None, help='where the files are written (default: a temporary directory)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'reassign_front_bench.json'))
    ap.add_argument('--files-only', action='store_true', help='write the files and stop (a rehearsal without a device)')
    args = ap.parse_args()
    sizes = [int(k) for k in args.keys.split(',')]
    record = {'contigs': args.contigs, 'groups': args.groups, 'repeats': args.repeats,
              'yardstick': {'fasta': 'cluster.parse_fasta (the per-line loop) on the same file', 'tables': 'parse_pickle + parse_link_dict of '
                            'patch_reassign(R, rounds=True, pickle=True) (resident=False) on the same file'}, 'sizes': {}}
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        fasta, prefix = os.path.join(tmp, 'asm.fa'), os.path.join(tmp, 'asm_prefix.fa')
        t0 = clock()
        bases, prefix_ctgs, prefix_bases = write_assembly(fasta, args.contigs, args.bases, prefix_path=prefix, prefix_bases=min(args.yardstick_bases, args.bases))
        record['assembly'] = {'bases': bases, 'file_bytes': os.path.getsize(fasta), 'write_s': clock() - t0, 'yardstick_contigs': prefix_ctgs,
                              'yardstick_bases': prefix_bases}
        print('assembly', json.dumps(record['assembly']), flush=True)
        if args.files_only:
            return
        import reassign_bench as rb
        from haphic_amd import _lib
        seams, parent = stand_in(True, True), stand_in(False, False)
        time_fasta(seams, prefix)                                                       # warm: code objects, pool blocks, pinned buffers
        ours, theirs, fa_dict = [], [], None
        for r in range(args.repeats):
            got, fa_dict = time_fasta(seams, fasta)
            ours.append(got)
            del fa_dict
            want, ref_dict = time_fasta(parent, prefix)
            theirs.append(want)
            if r == 0:                                                                 # the same table on the contigs both read
                first, fa_dict = time_fasta(seams, prefix)
                assert list(fa_dict) == list(ref_dict) and all(fa_dict[c][1:] == ref_dict[c][1:] for c in ref_dict), 'the seam and the yardstick disagree'
                del fa_dict, first
            del ref_dict
        profiled, fa_dict = time_fasta(seams, fasta, profile=True)                       # one more run, not timed: the events slow the host
        del fa_dict
        scale = bases / prefix_bases
        record['fasta'] = {'seam': dict(spread([x['s'] for x in ours]), kernel_ms=profiled['kernel_ms'], contigs=ours[-1]['contigs'], bases=ours[-1]['bases'],
                                        re_sites=ours[-1]['re_sites']),
                           'yardstick_on_prefix': dict(spread([x['s'] for x in theirs]), bases=theirs[-1]['bases']),
                           'yardstick': dict({k: v * scale for k, v in spread([x['s'] for x in theirs]).items() if k != 'runs'},
                                             how='measured' if prefix_bases >= bases else 'extrapolated: the prefix time by proportion of the bases')}
        print('fasta', json.dumps(record['fasta']), flush=True)
        _got, fa_dict = time_fasta(seams, fasta)

        job = rb.synth(args.contigs, max(sizes), args.groups, 0.15, 0.15)
        names = ['ctg%06d' % k for k in range(args.contigs)]
        gnames = ['group%d' % g for g in range(args.groups)]
        ctg_group_dict = {names[c]: (gnames[g] if g >= 0 else 'ungrouped') for c, g in enumerate(job['group'].tolist())}
        for n in sizes:
            n = min(n, len(job['fi']))
            path = os.path.join(tmp, 'full_links_%d.pkl' % n)
            _lib.write_link_pickle(path, job['fi'][:n], job['fj'][:n], job['links'][:n], names)
            time_tables(seams, path, fa_dict, ctg_group_dict)                          # warm
            ours, theirs = [], []
            for r in range(args.repeats):
                ours.append(time_tables(seams, path, fa_dict, ctg_group_dict))
                theirs.append(time_tables(parent, path, fa_dict, ctg_group_dict))
            assert ours[-1]['cells_checksum'] == theirs[-1]['cells_checksum'] and ours[-1]['key_fetches'] == 0
            entry = record['sizes'][str(n)] = {'file_bytes': os.path.getsize(path)}
            for label, runs in (('seam', ours), ('yardstick', theirs)):
                entry[label] = {'total': spread([x['s'] for x in runs]), 'parse_pickle': spread([x['parse_pickle_s'] for x in runs]),
                                'parse_link_dict': spread([x['parse_link_dict_s'] for x in runs]), 'tables': runs[-1]['tables'],
                                'key_fetches': runs[-1]['key_fetches']}
            entry['seam']['kernel_ms'] = time_tables(seams, path, fa_dict, ctg_group_dict, profile=True)['kernel_ms']      # not timed
            entry['whole_preparation_s'] = {'with_seams': record['fasta']['seam']['median_s'] + entry['seam']['total']['median_s'],
                                            'parent': record['fasta']['yardstick']['median_s'] + entry['yardstick']['total']['median_s'],
                                            'parent_fasta': record['fasta']['yardstick']['how']}
            os.remove(path)
            print(n, json.dumps(entry), flush=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1, sort_keys=True)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
