#!/usr/bin/env python3
"""Measures the verdict of `haphic sort` — fast sorting or ALLHiC per group, compare_fast_sort_and_allhic (HapHiC_sort.py :645-724) — on the device
(haphic_amd/csrc/hhx_sortverdict.hip behind haphic_amd/sort.py bind_verdict) and writes profiles/sort_verdict_bench.json.  A record, not a gate.

    python tools/sort_verdict_bench.py [--sizes 8,64,400,1000,4000,16000,41000] [--out profiles/sort_verdict_bench.json]
    python tools/sort_verdict_bench.py --reference-only --reference path/to/HapHiC/scripts [--reference-sizes 8,64,400,1000]     (no GPU)

The groups: synthetic tours that disagree (tests/sort_verdict_cases.shuffled: the ALLHiC tour is the fast-sort tour cut into blocks that are shuffled,
some reversed and flipped), group length / longest contig about 20, so the ratio rule lets them through and all n - 1 rotations are evaluated.  Per
size the device record holds the HIP-event time of the kernel, the wall time of the library call for all rotations, and the wall time of the whole
mirror: both tour files parsed, the lock taken, rotation 0 asked first and the rest after it, the log line formatted.  The reference checkout does not
exist where the GPU is, so the mirror runs over the parse_tours restatement of the tests (the last non-empty line of each file, split); the
reference's own function is timed where the checkout is, on one core, and carried over elsewhere, labelled `stored: true`.  The two records come
from different hosts: read them side by side.  For the small sizes the mirror is also timed over the host engine of the tests (O(n log n) per
rotation, pure Python) on the same host as the device: `crossing_vs_host_engine` is the size from which the device is the faster of the two.  The
yardstick for the wrapper's default is the reference's function, not that engine."""
import argparse
import json
import logging
import os
import platform
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import sort_verdict_cases as vc      # noqa: E402

SEED = 4242
SMALL = (2, 4, 8, 16, 24, 32, 48, 64, 96, 128)      # where the host engine and the device are compared


def group(n):
    return vc.shuffled('bench%d' % n, n, SEED + n, blocks=max(8, n // 40), ratio=20.0)


def box():
    return '%s, %d CPUs' % (platform.processor() or platform.machine(), os.cpu_count())


def best_of(fn, repeats):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return min(times), out


def mirror_wall(S, mirror, case, tmp, repeats):
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        fa_dict = vc.write_tours(case, case.name)
        return best_of(lambda: mirror(case.name, fa_dict), repeats)
    finally:
        os.chdir(cwd)


def device_record(sizes, repeats):
    from haphic_amd import _lib, sort
    S = vc.fake_module('sort_verdict_bench')
    S.logger.addHandler(logging.NullHandler())
    S.logger.propagate = False
    on_device, on_host = sort.bind_verdict(S), sort.bind_verdict(S, vc.stand_in)
    rows, small = [], []
    with tempfile.TemporaryDirectory() as tmp:
        mirror_wall(S, on_device, group(200), tmp, 1)                         # warm-up: library, pool, code object
        for n in sizes:
            case = group(n)
            value, lens = vc.values_of(case), [case.lens[c] for c, _ in case.fast]
            reps = repeats if n <= 4000 else 1
            _lib.sort_verdict_sums(value, lens)
            _lib.profile_enable(True)
            _lib.profile_reset()
            _sums, stats = _lib.sort_verdict_sums(value, lens, want_stats=True)
            kernel_ms, launches = _lib.profile_get('sort_verdict')
            _lib.profile_enable(False)
            call_s, sums = best_of(lambda: _lib.sort_verdict_sums(value, lens), reps)
            wall_s, verdict = mirror_wall(S, on_device, case, tmp, reps)
            row = {'n': n, 'rotations': n - 1, 'form': 'lds' if stats['lds_rotations'] else 'hbm', 'cell_bytes': stats['cell_bytes'],
                   'kernel_ms_hip_events': round(kernel_ms, 4), 'launches': launches, 'library_call_s': round(call_s, 6), 'mirror_s': round(wall_s, 6),
                   'verdict': bool(verdict), 'max_ratio': round(float(sums.max()) / sum(lens), 4)}
            if 1000 <= n <= 20000:                                            # both forms at the same size: where the default seam stands
                for form, knob in (('lds', 1 << 40), ('hbm', 0)):
                    _lib.tune('sort_verdict_lds_n', knob)
                    row['library_call_s_%s_form' % form] = round(best_of(lambda: _lib.sort_verdict_sums(value, lens), 2)[0], 6)
                _lib.tune('sort_verdict_lds_n', None)
            rows.append(row)
            print(json.dumps(row), flush=True)
        for n in SMALL:
            case = group(n)
            d, vd = mirror_wall(S, on_device, case, tmp, 20)
            h, vh = mirror_wall(S, on_host, case, tmp, 20)
            assert vd == vh
            small.append({'n': n, 'mirror_device_s': round(d, 6), 'mirror_host_engine_s': round(h, 6)})
    crossing = next((r['n'] for k, r in enumerate(small) if all(q['mirror_device_s'] <= q['mirror_host_engine_s'] for q in small[k:])), None)
    return {'what': 'synthetic disagreeing tours (tests/sort_verdict_cases.shuffled, group length / longest contig = 20): every rotation evaluated',
            'box': box(), 'sizes': rows, 'small_sizes_same_host': small, 'crossing_vs_host_engine': crossing,
            'note': 'kernel_ms_hip_events: HIP events around the one launch of all n - 1 rotations; library_call_s: _lib.sort_verdict_sums from Python, '
                    'ranking, allocation, uploads, the copy of the sums and the synchronisation included (best of %d up to n = 4000, one run above); mirror_s: '
                    'bind_verdict end to end over the parse_tours restatement of tests/sort_verdict_cases.py: two tour files read, the lock, rotation 0 '
                    'and then the rest in a second call, the threshold loop, the log line; library_call_s_lds_form / _hbm_form: the same call with hhx_tune "sort_verdict_lds_n" at its '
                    'upper clamp / at 0; crossing_vs_host_engine: the smallest n from which the mirror over the device is no slower than the mirror over '
                    'tests/sort_verdict_cases.stand_in at every larger small size, same host, best of 20' % repeats}


def reference_record(scripts, sizes):
    """the reference's own compare_fast_sort_and_allhic, unmodified, on the same groups; one core"""
    from tests import sort_cases
    S = sort_cases.load_reference_sort(scripts, '_haphic_sort_reference_verdict_bench')
    for lg in (S.logger, S.parse_tours.__globals__['logger']):
        lg.addHandler(logging.NullHandler())
        lg.propagate = False
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for n in sizes:
            case = group(n)
            wall_s, verdict = mirror_wall(S, S.compare_fast_sort_and_allhic, case, tmp, 5 if n <= 64 else 1)
            rows.append({'n': n, 'function_s': round(wall_s, 6), 'verdict': bool(verdict)})
            print(json.dumps(rows[-1]), flush=True)
    return {'what': 'HapHiC_sort.compare_fast_sort_and_allhic, unmodified, on the same groups (tour parsing included); one core; best of 5 up to n = 64, '
                    'one run above', 'stored': False, 'box': box(), 'sizes': rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--sizes', default='8,64,400,1000,4000,16000,41000', help='16000: past the default LDS seam (4095); 41000: past what fits the LDS at all (40959)')
    ap.add_argument('--reference-sizes', default='8,64,400,1000')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sort_verdict_bench.json'))
    ap.add_argument('--reference', default=os.environ.get('HAPHIC_REFERENCE'), help="HapHiC's scripts/ directory: time its function too")
    ap.add_argument('--reference-only', action='store_true', help='no GPU: the reference record alone (the other records of --out are kept)')
    args = ap.parse_args()
    res = {}
    for p in (args.out, os.path.join(ROOT, 'profiles', 'sort_verdict_bench.json')):
        if os.path.exists(p):
            with open(p) as f:
                res = json.load(f)
            break
    if not args.reference_only:
        res['device'] = device_record([int(x) for x in args.sizes.split(',')], args.repeats)
    if args.reference and os.path.isdir(args.reference):
        res['reference'] = reference_record(args.reference, [int(x) for x in args.reference_sizes.split(',')])
    elif 'reference' in res:
        res['reference']['stored'] = True
    if 'device' in res and 'reference' in res:
        ref = {r['n']: r['function_s'] for r in res['reference']['sizes']}
        res['side_by_side'] = [{'n': r['n'], 'reference_function_s': ref[r['n']], 'mirror_s': r['mirror_s'], 'library_call_s': r['library_call_s']}
                               for r in res['device']['sizes'] if r['n'] in ref]
        loses = [r['n'] for r in res['side_by_side'] if r['mirror_s'] > r['reference_function_s']]
        res['cut_over'] = {'sizes_where_the_mirror_is_slower_than_the_reference_function': loses,
                           'bound': 'none: every group goes to the device' if not loses else 'needed below n = %s' % res['device']['crossing_vs_host_engine']}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res.get('side_by_side', res.get('reference'))))


if __name__ == '__main__':
    main()
