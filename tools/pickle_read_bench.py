#!/usr/bin/env python3
"""Measures full_links.pkl -> arrays on the device (_lib.read_link_pickle, csrc/hhx_pickleread.hip) against the parent's path — pickle.load, then
cluster._dict_arrays inside parse_link_dict — and writes profiles/pickle_read_bench.json.  A record, not a gate.

    python tools/pickle_read_bench.py [--keys 5000000,134000000] [--dict-keys 5000000]          (one MI355X, one session)

The table is the synthetic one of tools/reassign_bench.py (100 000 contigs, 32 groups).  Per size and dialect — "library": the file
hhx_write_link_pickle writes (what `python -m haphic_amd cluster` leaves behind); "python": pickle.dump of the dict with a str object of its own in
every key (what `haphic cluster` leaves behind: every name a literal again) — it records the file's bytes, the read of the file alone (the floor),
file -> arrays wall time with the kernels' time by the library's HIP events, and file -> parse_link_dict done through the seams of
patch_reassign(R, rounds=True, pickle=True).  The yardstick is the same from the same file with pickle=False: pickle.load + the parent's
parse_link_dict.  Both need a Python dict of every key, so they are taken at sizes up to --dict-keys; above that the python dialect is not
written at all and the parent's time is the --dict-keys figure scaled by the number of keys, labelled "extrapolated"."""
import argparse
import json
import logging
import os
import pickle
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
clock = time.perf_counter
KERNELS = ('pkl_boundaries', 'pkl_walk', 'pkl_names', 'pkl_keys')


def stand_in(pickle_seam):
    from haphic_amd import patch
    R = types.ModuleType('HapHiC_reassign_stand_in')
    R.logger = logging.getLogger('pickle_read_bench')

    def parse_pickle(fa_dict, pickle_file):                                       # :38-50
        with open(pickle_file, 'rb') as f:
            full_link_dict = pickle.load(f)
        return full_link_dict, None, None
    R.parse_pickle = parse_pickle
    for name in ('parse_link_dict', 'run_reassignment', 'agglomerative_hierarchical_clustering', 'split_clm_file'):
        setattr(R, name, None)
    patch.patch_reassign(R, rounds=True, pickle=pickle_seam)
    return R


def file_to_tables(path, ctg_group_dict, pickle_seam):
    R = stand_in(pickle_seam)
    t0 = clock()
    link_dict = R.parse_pickle({}, path)[0]
    t1 = clock()
    tables = R.parse_link_dict(link_dict, ctg_group_dict)
    t2 = clock()
    out = {'parse_pickle_s': t1 - t0, 'parse_link_dict_s': t2 - t1, 'total_s': t2 - t0, 'full_link_dict': type(link_dict).__name__,
           'tables': type(tables[0]).__name__, 'frozen_after': bool(getattr(link_dict, 'frozen', False))}
    del tables, link_dict
    return out


def measure(path, ctg_group_dict, with_parent):
    from haphic_amd import _lib
    out = {'file_bytes': os.path.getsize(path)}
    buf = bytearray(out['file_bytes'])
    for label in ('read_file_first_s', 'read_file_s'):
        t0 = clock()
        with open(path, 'rb', buffering=0) as f:
            got, view = 0, memoryview(buf)
            while got < len(buf):
                got += f.readinto(view[got:got + (64 << 20)])
        out[label] = clock() - t0
    del buf
    _lib.read_link_pickle(path)                                                    # warm: pool blocks, pinned buffers
    _lib.profile_enable(True)
    _lib.profile_reset()
    t0 = clock()
    arrays = _lib.read_link_pickle(path)
    out['file_to_arrays_s'] = clock() - t0
    out['kernel_ms'] = {k: _lib.profile_get(k)[0] for k in KERNELS}
    out['kernel_ms']['total'] = sum(out['kernel_ms'].values())
    _lib.profile_enable(False)
    out['keys'], out['names'] = len(arrays[0]), len(arrays[4])
    del arrays
    out['device_seams'] = file_to_tables(path, ctg_group_dict, True)
    if with_parent:
        out['parent_seams'] = file_to_tables(path, ctg_group_dict, False)
    return out


def main():
    import reassign_bench as rb
    from haphic_amd import _lib
    ap = argparse.ArgumentParser()
    ap.add_argument('--contigs', type=int, default=100000)
    ap.add_argument('--groups', type=int, default=32)
    ap.add_argument('--keys', default='5000000,134000000')
    ap.add_argument('--dict-keys', type=int, default=5000000)
    ap.add_argument('--dir', default=None, help='where the pickles are written (default: a temporary directory)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pickle_read_bench.json'))
    args = ap.parse_args()
    sizes = [int(k) for k in args.keys.split(',')]
    job = rb.synth(args.contigs, max(sizes), args.groups, 0.15, 0.15)
    names = ['ctg%06d' % k for k in range(args.contigs)]
    gnames = ['group%d' % g for g in range(args.groups)]
    ctg_group_dict = {names[c]: (gnames[g] if g >= 0 else 'ungrouped') for c, g in enumerate(job['group'].tolist())}
    record = {'contigs': args.contigs, 'groups': args.groups, 'yardstick': 'pickle.load + the parent\'s parse_link_dict (patch_reassign(R, rounds=True)) '
              'on the same file, same box, same session', 'sizes': {}}
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        for n in sizes:
            n = min(n, len(job['fi']))
            fi, fj, links = job['fi'][:n], job['fj'][:n], job['links'][:n]
            entry = record['sizes'][str(n)] = {}
            path = os.path.join(tmp, 'library_%d.pkl' % n)
            _lib.write_link_pickle(path, fi, fj, links, names)
            entry['library'] = measure(path, ctg_group_dict, n <= args.dict_keys)
            os.remove(path)
            print(n, 'library', json.dumps(entry['library']), flush=True)
            if n <= args.dict_keys:
                path = os.path.join(tmp, 'python_%d.pkl' % n)
                t0 = clock()
                d = dict(zip(zip(map('ctg%06d'.__mod__, fi.tolist()), map('ctg%06d'.__mod__, fj.tolist())), links.tolist()))
                build = clock() - t0
                from collections import defaultdict
                with open(path, 'wb') as f:
                    pickle.dump(defaultdict(int, d), f, 4)
                del d
                entry['python'] = measure(path, ctg_group_dict, True)
                entry['python']['dict_build_s'] = build
                os.remove(path)
                print(n, 'python', json.dumps(entry['python']), flush=True)
            else:
                entry['python'] = 'not written: the pickler needs the dict of every key'
        base = record['sizes'].get(str(min(args.dict_keys, len(job['fi']))))
        for n, entry in record['sizes'].items():
            if base and 'parent_seams' not in entry['library'] and 'parent_seams' in base['library']:
                entry['library']['parent_seams_extrapolated'] = {'total_s': base['library']['parent_seams']['total_s'] * int(n) / base['library']['keys'],
                                                                 'from_keys': base['library']['keys'], 'how': 'by proportion of the keys'}
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1, sort_keys=True)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
