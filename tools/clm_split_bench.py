#!/usr/bin/env python3
"""Measures the CLM split of `haphic reassign` (haphic_amd/csrc/hhx_clmsplit.hip) on a synthetic paired_links.clm and writes
profiles/clm_split_bench.json.  A record, not a gate.

    python tools/clm_split_bench.py [--gb 2] [--dir /dev/shm] [--chunk-mb 64] [--out profiles/clm_split_bench.json]
    python tools/clm_split_bench.py --reference-only --reference path/to/HapHiC/scripts      (no GPU: times the reference alone)

The file: 100 000 contig names in 40 groups (a tenth of the contigs in none), one line per contig pair and orientation as output_clm
writes them ("ctgA+ ctgB-\\t<n>\\t<d1> <d2> ..."), the number of links per line drawn from a log-normal like the C3 job's link table
(median ~4, mean ~14, a tail into the thousands), 60 % of the lines inside one group, plus a handful of lines of 3-6 MB.
Measured: the end-to-end rate of hhx_clm_split_file (pinned read-ahead -> device -> writer lanes, files complete), the HIP-event
time of every kernel class against the host -> device and device -> host copies of the same chunks, and the rate of plainly writing
the same output bytes to the same directory in the same session.  For scale the reference's own split_clm_file is timed where its
checkout exists, on a prefix of at most 200 MB of the same file; elsewhere that record is carried over, labelled `stored: true`."""
import argparse
import json
import os
import platform
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_CONTIGS, N_GROUPS, HEAD = 100_000, 40, 24
KERNELS = ('clm_breaks', 'clm_parse', 'clm_partition', 'clm_gather')
COPIES = ('clm_h2d', 'clm_d2h')


def table():
    names = ['ctg%06d' % k for k in range(N_CONTIGS)]
    group = (np.arange(N_CONTIGS) % N_GROUPS).astype(np.int32)
    group[np.arange(N_CONTIGS) % 10 == 9] = -1
    return names, group


def synth(n_bytes, seed=11, n_huge=6):
    """-> uint8 array of about n_bytes: lines of HEAD + 8 * links bytes ("ctg000123+ ctg000456-\\t7\\t" + links of 7 digits and a space)"""
    rng = np.random.default_rng(seed)
    links = []
    size = 0
    while size < n_bytes:
        n = np.minimum(np.floor(rng.lognormal(1.5, 1.5, 1 << 20)).astype(np.int64) + 1, 100_000)
        links.append(n)
        size += int((HEAD + 8 * n).sum())
    links = np.concatenate(links)
    lens = HEAD + 8 * links
    keep = int(np.searchsorted(np.cumsum(lens), n_bytes)) + 1
    links, lens = links[:keep], lens[:keep]
    if n_huge:                                                       # a handful of contig pairs with hundreds of thousands of links: lines of 3-6 MB
        at = rng.choice(keep, n_huge, replace=False)
        lens[at] = HEAD + 8 * rng.integers(400_000, 800_000, n_huge)
    ends = np.cumsum(lens)
    starts = ends - lens
    total = int(ends[-1])
    pool = rng.integers(ord('1'), ord('9') + 1, 1 << 24, dtype=np.uint8)
    pool[7::8] = ord(' ')
    out = np.tile(pool, total // pool.size + 1)[:total]
    a = rng.integers(0, N_CONTIGS, keep)
    same = rng.random(keep) < 0.6
    b = np.where(same, (a + N_GROUPS * rng.integers(1, 2000, keep)) % N_CONTIGS, rng.integers(0, N_CONTIGS, keep))
    head = np.empty((keep, HEAD), np.uint8)
    head[:] = np.frombuffer(b'ctg000000+ ctg000000-\t7\t', np.uint8)
    for col, ids in ((3, a), (14, b)):
        for d in range(6):
            head[:, col + d] = ord('0') + (ids // 10 ** (5 - d)) % 10
    head[:, 9] = np.where(rng.random(keep) < 0.5, ord('+'), ord('-'))
    head[:, 20] = np.where(rng.random(keep) < 0.5, ord('+'), ord('-'))
    for lo in range(0, keep, 1 << 20):                               # (blocks: the index array of a whole file would take 8 x its heads)
        hi = min(lo + (1 << 20), keep)
        out[(starts[lo:hi, None] + np.arange(HEAD)[None, :]).ravel()] = head[lo:hi].ravel()
    out[ends - 1] = ord('\n')
    return out, {'lines': keep, 'bytes': total, 'median_line_bytes': float(np.median(lens)), 'mean_line_bytes': float(lens.mean()),
                 'max_line_bytes': int(lens.max()), 'lines_over_1MB': int((lens > (1 << 20)).sum())}


def time_reference(scripts, text, names, group, work_dir, limit=200 << 20):
    """the reference's own split_clm_file on the lines that fit `limit` bytes"""
    from tests.golden.make_golden_clm_split import load_reference_reassign
    R = load_reference_reassign(scripts)
    cut = min(len(text), limit)
    cut = int(np.flatnonzero(text[:cut] == 10)[-1]) + 1
    d = tempfile.mkdtemp(dir=work_dir)
    cwd = os.getcwd()
    try:
        clm = os.path.join(d, 'prefix.clm')
        text[:cut].tofile(clm)
        group_ctg_dict = {'g%d' % g: [set(), 0] for g in range(N_GROUPS)}
        ctg_group_dict = {n: 'g%d' % g for n, g in zip(names, group.tolist()) if g >= 0}
        os.chdir(d)
        t0 = time.perf_counter()
        R.split_clm_file(clm, group_ctg_dict, ctg_group_dict, 'reassigned_groups')
        dt = time.perf_counter() - t0
        kept = sum(os.path.getsize(os.path.join('split_clms', f)) for f in os.listdir('split_clms'))
    finally:
        os.chdir(cwd)
        shutil.rmtree(d, ignore_errors=True)
    return {'what': "HapHiC_reassign.split_clm_file on a prefix of the same file", 'stored': False, 'box': '%s, %d CPUs' % (platform.processor() or platform.machine(), os.cpu_count()),
            'bytes_in': cut, 'bytes_out': kept, 'lines': int((text[:cut] == 10).sum()), 'seconds': round(dt, 3), 'bytes_per_s': round(cut / dt)}


def run_split(_lib, clm, names, group, out_dir, chunk):
    shutil.rmtree(out_dir, ignore_errors=True)
    os.mkdir(out_dir)
    t0 = time.perf_counter()
    s = _lib.ClmSplit(names, group, [os.path.join(out_dir, 'g%d.clm' % g) for g in range(N_GROUPS)])
    try:
        s.push_file(clm, chunk, 4)
        lines, kept, per = s.finish()
        stats = s.stats()
    finally:
        s.close()
    return time.perf_counter() - t0, lines, kept, int(per.sum()), stats


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--gb', type=float, default=2.0)
    ap.add_argument('--dir', default='/dev/shm' if os.path.isdir('/dev/shm') else None, help='where the file and its parts go (a RAM disk)')
    ap.add_argument('--chunk-mb', type=int, default=64)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'clm_split_bench.json'))
    ap.add_argument('--reference', default=os.environ.get('HAPHIC_REFERENCE'), help="HapHiC's scripts/ directory: time its split_clm_file too")
    ap.add_argument('--reference-only', action='store_true', help='no GPU: the reference record alone (the other records of --out are kept)')
    args = ap.parse_args()
    stored_path = os.path.join(ROOT, 'profiles', 'clm_split_bench.json')
    res = {}
    for p in (args.out, stored_path):
        if os.path.exists(p):
            with open(p) as f:
                res = json.load(f)
            break
    names, group = table()
    work = tempfile.mkdtemp(prefix='clm_split_bench_', dir=args.dir)
    try:
        if args.reference_only:
            text, shape = synth(min(int(args.gb * 2 ** 30), 210 << 20), n_huge=2)
            res['reference'] = time_reference(args.reference, text, names, group, work)
            res['reference']['file'] = shape
        else:
            from haphic_amd import _lib
            text, shape = synth(int(args.gb * 2 ** 30))
            clm = os.path.join(work, 'paired_links.clm')
            text.tofile(clm)
            chunk = args.chunk_mb << 20
            out_dir = os.path.join(work, 'split_clms')
            run_split(_lib, clm, names, group, out_dir, chunk)                                   # warm-up: pinned buffers, pool, page cache
            runs = [run_split(_lib, clm, names, group, out_dir, chunk) for _ in range(2)]
            dt, lines, kept, bytes_out, stats = min(runs, key=lambda r: r[0])
            _lib.profile_reset()
            _lib.profile_enable(True)
            try:
                dt_prof = run_split(_lib, clm, names, group, out_dir, chunk)[0]
            finally:
                _lib.profile_enable(False)
            n_chunks = -(-shape['bytes'] // chunk)
            events = {k: dict(zip(('ms', 'records'), _lib.profile_get(k))) for k in KERNELS + COPIES}
            kernel_ms, copy_ms = sum(events[k]['ms'] for k in KERNELS), sum(events[k]['ms'] for k in COPIES)
            # the same output bytes, written plainly: one file after the other from memory, same directory
            outs = [open(os.path.join(out_dir, 'g%d.clm' % g), 'rb').read() for g in range(N_GROUPS)]
            plain = os.path.join(work, 'plain')
            os.mkdir(plain)
            t0 = time.perf_counter()
            for g, data in enumerate(outs):
                with open(os.path.join(plain, 'g%d.clm' % g), 'wb') as f:
                    f.write(data)
            dt_write = time.perf_counter() - t0
            t0 = time.perf_counter()
            with open(clm, 'rb') as f:
                while f.read(64 << 20):
                    pass
            dt_read = time.perf_counter() - t0
            res.update({
                'what': 'hhx_clm_split_file on a synthetic paired_links.clm (tools/clm_split_bench.py)', 'box': '%s, %d CPUs' % (platform.processor() or platform.machine(), os.cpu_count()),
                'directory': args.dir, 'file': shape, 'groups': N_GROUPS, 'contigs': N_CONTIGS, 'chunk_bytes': chunk, 'chunks': n_chunks,
                'end_to_end': {'seconds': round(dt, 3), 'seconds_of_both_runs': [round(r[0], 3) for r in runs], 'bytes_in': shape['bytes'], 'bytes_out': bytes_out,
                               'bytes_in_per_s': round(shape['bytes'] / dt), 'lines': lines, 'lines_kept': kept, 'counters': stats},
                'hip_events': {'note': 'totals over all chunks of one profiled run; clm_partition spans the radix sort and two scans with their host synchronisations, so it '
                                       'holds idle gaps between launches; copies: clm_h2d = chunk to the device, clm_d2h = output buffer to pinned memory',
                               'profiled_run_seconds': round(dt_prof, 3), 'by_class': events, 'kernels_ms': round(kernel_ms, 3), 'copies_ms': round(copy_ms, 3),
                               'kernels_ms_per_chunk': round(kernel_ms / n_chunks, 3), 'copies_ms_per_chunk': round(copy_ms / n_chunks, 3),
                               'kernels_over_copies': round(kernel_ms / copy_ms, 3) if copy_ms else None},
                'plain_write': {'what': 'the same output bytes written file after file from memory into the same directory', 'bytes': bytes_out, 'seconds': round(dt_write, 3),
                                'bytes_per_s': round(bytes_out / dt_write) if dt_write else None},
                'plain_read': {'what': 'the input file read once in 64 MB pieces', 'bytes': shape['bytes'], 'seconds': round(dt_read, 3), 'bytes_per_s': round(shape['bytes'] / dt_read)},
            })
            if args.reference and os.path.isdir(args.reference):
                res['reference'] = time_reference(args.reference, text, names, group, work)
            elif 'reference' in res:
                res['reference']['stored'] = True
    finally:
        shutil.rmtree(work, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps({k: res[k] for k in ('end_to_end', 'hip_events', 'plain_write', 'reference') if k in res}))


if __name__ == '__main__':
    main()
