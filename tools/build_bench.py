#!/usr/bin/env python3
"""Measures `haphic build` on the device (haphic_amd/csrc/hhx_fasta.hip, haphic_amd/scaffolds.py) on a synthetic assembly and writes
profiles/build_bench.json.  A record, not a gate.

    python tools/build_bench.py [--mb 3000] [--dir /dev/shm] [--out profiles/build_bench.json]
    python tools/build_bench.py --reference-only --reference path/to/HapHiC/scripts [--mb 200]      (no GPU: times the reference alone)

The assembly: contigs of 100 kb in lines of 60 columns (a tenth of the bases soft-masked), ten tours over nine tenths of the contigs with random
orientations, the rest unanchored; --Ns 100, --max_width 60.  Measured on the device: the wall time from the file to the FastaTable, the HIP-event
time of every kernel class of the reader and of the writer with the bytes they move, the wall time from FastaTable + tours to the complete
scaffolds.fa (and both AGP files), and the rate of plainly writing the same output bytes to the same directory in the same session — the floor of
the step.  For scale the reference's own parse_fasta and build_final_scaffolds are timed on one core where its checkout is given, at a size that
finishes in seconds; elsewhere that record is carried over from the existing file, labelled `stored: true`."""
import argparse
import json
import os
import platform
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONTIG, COLUMNS, N_TOURS = 100_000, 60, 10
READER_KERNELS = ('fa_high', 'fa_breaks', 'fa_classify', 'fa_tables', 'fa_copy')
HBM_PEAK = 8.0e12                 # bytes per second, the MI355X's nominal HBM3E rate


def synth(directory, n_mb, seed=3):
    """writes asm.fa of about n_mb MB and the tour files -> (fasta path, tour paths, contigs)"""
    rng = np.random.default_rng(seed)
    n_ctg = max(int(n_mb * 1e6) // CONTIG, N_TOURS + 2)
    pool = np.frombuffer(b'ACGT', np.uint8)[rng.integers(0, 4, 1 << 24)]
    mask = rng.random(1 << 24) < 0.1
    pool = np.where(mask, pool | 0x20, pool).astype(np.uint8)
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
    order = rng.permutation(n_ctg)[:n_ctg * 9 // 10]
    tours = []
    for g, part in enumerate(np.array_split(order, N_TOURS)):
        tours.append(os.path.join(directory, 'group%d_bench.tour' % (g + 1)))
        with open(tours[-1], 'w') as f:
            f.write(' '.join('ctg%06d%s' % (k, '+-'[int(o)]) for k, o in zip(part.tolist(), rng.integers(0, 2, part.size))) + '\n')
    return fasta, tours, n_ctg


def args_for(fasta, tours):
    return types.SimpleNamespace(fasta=fasta, raw_fasta=fasta, alignments='aln.bam', tours=tours, corrected_ctgs=None, Ns=100, max_width=COLUMNS,
                                 sort_by_input=False, keep_letter_case=False, prefix='scaffolds')


def box():
    return '{}, {} CPUs'.format(platform.machine(), os.cpu_count())


def in_dir(directory, fn):
    cwd = os.getcwd()
    os.chdir(directory)
    try:
        return fn()
    finally:
        os.chdir(cwd)


def reference_record(scripts, n_mb, directory):
    """the reference's own functions, one core"""
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    from make_golden_build import load_reference_build
    B = load_reference_build(scripts)
    with tempfile.TemporaryDirectory(dir=directory) as tmp:
        fasta, tours, n_ctg = synth(tmp, n_mb)
        args = args_for(fasta, tours)
        t0 = time.perf_counter()
        fa_dict = B.parse_fasta(fasta)
        t_parse = time.perf_counter() - t0
        tour_dict, output_ctgs = B.parse_tours(tours, fa_dict)
        t0 = time.perf_counter()
        in_dir(tmp, lambda: B.build_final_scaffolds(tour_dict, fa_dict, output_ctgs, set(), args))
        t_build = time.perf_counter() - t0
        return {'what': 'HapHiC_cluster.parse_fasta and HapHiC_build.build_final_scaffolds on the same generator, one core', 'stored': False, 'box': box(),
                'contigs': n_ctg, 'fasta_bytes': os.path.getsize(fasta), 'scaffolds_fa_bytes': os.path.getsize(os.path.join(tmp, 'scaffolds.fa')),
                'parse_fasta_seconds': round(t_parse, 3), 'build_final_scaffolds_seconds': round(t_build, 3)}


def device_record(n_mb, directory):
    from haphic_amd import _lib, scaffolds
    from tests import build_cases as bc
    rec = {'what': 'haphic build on the device: scaffolds.parse_fasta and scaffolds.build_final_scaffolds on a synthetic assembly (tools/build_bench.py)',
           'box': box(), 'directory': directory, 'hbm_peak_bytes_per_s': HBM_PEAK}
    with tempfile.TemporaryDirectory(dir=directory) as tmp:
        fasta, tours, n_ctg = synth(tmp, n_mb)
        args = args_for(fasta, tours)
        n_text = os.path.getsize(fasta)
        rec.update(contigs=n_ctg, contig_bytes=CONTIG, columns=COLUMNS, tours=N_TOURS, Ns=args.Ns, max_width=args.max_width, fasta_bytes=n_text)
        _lib.Fasta(b'>a\nACGT\n').close()                          # the device and the library are up
        walls = []
        for _ in range(2):
            t0 = time.perf_counter()
            table = scaffolds.parse_fasta(fasta)
            walls.append(round(time.perf_counter() - t0, 3))
            if len(walls) < 2:
                table.engine.close()
        n_seq = int(table.lengths.sum())
        rec['file_to_fasta_table'] = {'seconds': min(walls), 'seconds_of_both_runs': walls, 'bytes_in_per_s': int(n_text / min(walls)), 'sequence_bytes': n_seq}
        tour_dict, output_ctgs = bc.parse_tours(tours, table)
        walls, emit_walls = [], []
        emit = table.engine.emit

        def timed_emit(*a):                                          # the one library call inside the mirror, timed on its own
            t0 = time.perf_counter()
            n = emit(*a)
            emit_walls.append(round(time.perf_counter() - t0, 3))
            return n
        table.engine.emit = timed_emit
        for _ in range(2):
            t0 = time.perf_counter()
            in_dir(tmp, lambda: scaffolds.build_final_scaffolds(tour_dict, table, output_ctgs, set(), args))
            walls.append(round(time.perf_counter() - t0, 3))
        table.engine.emit = emit
        out_path = os.path.join(tmp, 'scaffolds.fa')
        n_out = os.path.getsize(out_path)
        t0 = time.perf_counter()
        emit(os.path.join(tmp, 'one_record.fa'), ['ctg000000'], [0, 1], [0], [1], 100, COLUMNS)
        tiny = round(time.perf_counter() - t0, 3)
        rec['fasta_table_to_files'] = {'seconds': min(walls), 'seconds_of_both_runs': walls, 'scaffolds_fa_bytes': n_out, 'bytes_out_per_s': int(n_out / min(walls)),
                                       'hhx_fasta_emit_seconds_of_both_runs': emit_walls, 'hhx_fasta_emit_seconds_one_100kb_record': tiny}
        # the kernels alone, by HIP events, in a run of their own
        table.engine.close()
        _lib.profile_enable(True)
        _lib.profile_reset()
        table = scaffolds.parse_fasta(fasta)
        _lib.load().hhx_synchronize()
        moved = {'fa_high': n_text, 'fa_breaks': 2 * n_text, 'fa_classify': None, 'fa_tables': None, 'fa_copy': 2 * n_seq}
        events = {}
        for k in READER_KERNELS:
            ms, n = _lib.profile_get(k)
            events[k] = {'ms': round(ms, 3), 'launches': n}
            if moved[k] and ms > 0:
                events[k].update(bytes_moved=moved[k], bytes_per_s=int(moved[k] / (ms / 1e3)), hbm_fraction=round(moved[k] / (ms / 1e3) / HBM_PEAK, 3))
        reader_ms = sum(e['ms'] for e in events.values())
        _lib.profile_reset()
        in_dir(tmp, lambda: scaffolds.build_final_scaffolds(tour_dict, table, output_ctgs, set(), args))
        ms, n = _lib.profile_get('fa_emit')
        _lib.profile_enable(False)
        emit_moved = n_seq + n_out
        events['fa_emit'] = {'ms': round(ms, 3), 'launches': n, 'bytes_moved': emit_moved, 'bytes_per_s': int(emit_moved / (ms / 1e3)) if ms > 0 else None,
                             'hbm_fraction': round(emit_moved / (ms / 1e3) / HBM_PEAK, 3) if ms > 0 else None}
        rec['hip_events'] = {'note': 'bytes_moved: text bytes read by fa_high, read twice by the two break passes (fa_breaks), sequence bytes read and written by '
                                     'fa_copy (its tables not counted), sequence bytes read plus file bytes written by fa_emit; fa_classify and fa_tables touch the '
                                     'line ends and 56 bytes of tables per line', 'reader_ms': round(reader_ms, 3), 'kernels': events}
        # the floor: the same bytes from host memory to a file in the same directory
        with open(out_path, 'rb') as f:
            data = f.read()
        walls = []
        for k in range(2):
            t0 = time.perf_counter()
            with open(os.path.join(tmp, 'plain_%d.fa' % k), 'wb') as f:
                f.write(data)
            walls.append(round(time.perf_counter() - t0, 3))
            os.remove(os.path.join(tmp, 'plain_%d.fa' % k))
        rec['plain_write'] = {'seconds': min(walls), 'seconds_of_both_runs': walls, 'bytes_per_s': int(n_out / min(walls))}
        rec['files_over_plain_write'] = round(rec['fasta_table_to_files']['seconds'] / rec['plain_write']['seconds'], 2)
        table.engine.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mb', type=float, default=None, help='size of the assembly in MB (default: 3000 on the device, 200 for the reference)')
    ap.add_argument('--dir', default='/dev/shm' if os.path.isdir('/dev/shm') else None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'build_bench.json'))
    ap.add_argument('--reference', default=None, help='the scripts/ directory of a HapHiC checkout')
    ap.add_argument('--reference-only', action='store_true')
    a = ap.parse_args()
    stored = {}
    for path in (a.out, os.path.join(ROOT, 'profiles', 'build_bench.json')):
        if os.path.exists(path):
            stored = json.load(open(path))
            break
    if a.reference_only:
        if not a.reference:
            raise SystemExit('--reference-only needs --reference DIR')
        rec = dict(stored)
        rec['reference'] = reference_record(a.reference, a.mb or 200, a.dir)
    else:
        rec = device_record(a.mb or 3000, a.dir)
        if a.reference:
            rec['reference'] = reference_record(a.reference, 200, a.dir)
        elif 'reference' in stored:
            rec['reference'] = dict(stored['reference'], stored=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps({k: v for k, v in rec.items() if k != 'hip_events'}))


if __name__ == '__main__':
    main()
