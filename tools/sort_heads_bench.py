#!/usr/bin/env python3
"""Measures the front of `haphic sort` — HT_links.pkl -> each group's sub_HT_dict (run() :898-923) — through the seams of patch_sort(S, heads=True)
on one MI355X and writes profiles/sort_heads_bench.json.  A record, not a gate.

    python tools/sort_heads_bench.py [--keys 5000000,220000000] [--dict-keys 5000000]                     (one MI355X, one session)
    python tools/sort_heads_bench.py --reference-only --reference path/to/HapHiC/scripts [--reference-groups 2]     (no GPU: see below)

The table is synthetic: 100 000 contigs in 32 planted groups, every key a pair of contig ends (80 % inside a group), names ctg%06d_H / _T.  Per
size and dialect — "library": the file hhx_write_link_pickle writes; "python": pickle.dump of the dict (Python's pickler) — it records
file -> table (the proxy's load), the fetch of the names and the name -> id dict, and per group the extraction by wall clock (slot and rank made on
the host included) and by the library's HIP events, split into the pass and the sort, under both settings of hhx_tune "heads_bitmap", alternating,
REPEATS times each.  The bytes of the pass (the two int32 ids of every key, plus id, slot and value traffic of the candidates, not counted) over its
event time is set against the float4-copy ceiling of the part (6.29 TB/s, DESIGN.md "Roofline"): a ratio, no threshold.  The results of both knob
settings are compared with each other and, for the first groups, with the numpy restatement of the rule on the same arrays (tests/sort_heads_cases.py
HostPickle: two groups up to --dict-keys, one above) — 'equal_to_the_numpy_engine' — and, where the checkout is, with the reference's.  Every size has
a table of its own (same seed), so a --reference-only record is about the same table as the device records of its size.  The record keeps the sums and
medians over all groups and the per-group medians of the first KEEP_GROUPS groups, not every sample.

The yardstick is the parent's path on the same file: pickle.load (timed here, in the same session) and then the reference's get_sub_HT_dict per
group.  That function lives in the HapHiC checkout, which does not exist where the GPU is: where --reference names it, it is timed on the same file
in the same process (a record 'reference' per group, all groups or the first --reference-groups of them, said so); --reference-only times it alone,
without a GPU, and keeps the other records of --out.  Above --dict-keys neither pickle.load nor the python dialect is run (both need a dict of every
key); the parent's figures there are the --dict-keys ones scaled by the number of keys and labelled "extrapolated"."""
import argparse
import gc
import json
import os
import pickle
import sys
import tempfile
import time
import types
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
clock = time.perf_counter
COPY_CEILING = 6.29e12               # bytes / s: the measured float4 copy of the part (DESIGN.md "Roofline")
REPEATS = 3
KEEP_GROUPS = 4


def synth(n_ctg, n_keys, n_groups, seed=3):
    """-> (name id of both ends [n_keys], values, group of every contig): distinct keys (lo end, hi end), lo contig < hi contig, in random order"""
    rng = np.random.default_rng(seed)
    group = (np.arange(n_ctg, dtype=np.int64) * n_groups // n_ctg).astype(np.int32)
    per = n_ctg // n_groups
    m = int(n_keys * 1.1) + 1000
    a = rng.integers(0, n_ctg, m)
    inside = rng.random(m) < 0.8
    b = np.where(inside, np.minimum(n_ctg - 1, group[a].astype(np.int64) * per + rng.integers(0, per, m)), rng.integers(0, n_ctg, m))
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    code = ((lo * n_ctg + hi) << 2 | rng.integers(0, 4, m))[lo != hi]
    del a, b, lo, hi, inside
    code = np.unique(code)
    code = code[rng.permutation(code.size)[:n_keys]]
    pair, ends = code >> 2, code & 3
    fi, fj = (2 * (pair // n_ctg) + (ends >> 1)).astype(np.int32), (2 * (pair % n_ctg) + (ends & 1)).astype(np.int32)
    links = np.where(group[fi >> 1] == group[fj >> 1], rng.integers(5, 60, fi.size), rng.integers(1, 10, fi.size)).astype(np.int64)
    return fi, fj, links, group


def groups_of(group, n_groups, seed=4):
    """the contigs of every group in the order parse_group returns them: by a seeded length, descending"""
    rng = np.random.default_rng(seed)
    length = rng.integers(10_000, 5_000_000, group.size)
    out = []
    for g in range(n_groups):
        members = np.flatnonzero(group == g)
        out.append(['ctg%06d' % c for c in members[np.argsort(-length[members], kind='stable')].tolist()])
    return out


def stand_in(heads):
    """what patch_sort reads of HapHiC_sort; with heads=False the parent's front: pickle.load"""
    from haphic_amd import patch

    def missing(*a, **k):
        raise RuntimeError('the reference checkout is not here: this call was handed back')
    S = types.SimpleNamespace(**{name: missing for name in list(patch.SORT_SEAMS) + ['get_sub_HT_dict']})
    S.pickle, S.Pool = pickle, object
    patch.patch_sort(S, heads=heads)
    return S


def device_front(path, groups, knobs, keep):
    """file -> table -> every group, the knob settings alternating -> (record, {group index: (i, j, w)} for the groups in keep)"""
    from haphic_amd import _lib
    S = stand_in(True)
    t0 = clock()
    with open(path, 'rb') as f:
        table = S.pickle.load(f)
    out = {'file_to_table_s': clock() - t0, 'table': type(table).__name__, 'keys': len(table)}
    t0 = clock()
    out['names'] = len(table.name_ids())
    out['names_and_ids_s'] = clock() - t0
    S.get_sub_HT_dict(groups[0], table)                                          # warm: code objects, pool blocks
    _lib.profile_enable(True)
    kept, per_group = {}, []
    for g, ctgs in enumerate(groups):
        rec = {'contigs': len(ctgs)}
        for knob in knobs:
            rec['bitmap_%d' % knob] = {'wall_s': [], 'pass_ms': [], 'sort_ms': []}
        for _ in range(REPEATS):
            for knob in knobs:
                _lib.tune('heads_bitmap', knob)
                _lib.profile_reset()
                t0 = clock()
                sub, index = S.get_sub_HT_dict(ctgs, table)
                wall = clock() - t0
                r = rec['bitmap_%d' % knob]
                r['wall_s'].append(wall)
                r['pass_ms'].append(_lib.profile_get('heads_pass')[0])
                r['sort_ms'].append(_lib.profile_get('heads_sort')[0])
                rec['edges'] = len(sub)
                if g in keep:
                    if g in kept:
                        assert all(np.array_equal(x, y) for x, y in zip(kept[g], (sub.i, sub.j, sub.w))), 'the knob settings disagree'
                    kept[g] = (sub.i, sub.j, sub.w)
        per_group.append(rec)
    _lib.tune('heads_bitmap', None)
    _lib.profile_enable(False)
    assert table.frozen
    n_keys = out['keys']
    for knob in knobs:
        key = 'bitmap_%d' % knob
        med = lambda what: [float(np.median(r[key][what])) for r in per_group]                # noqa: E731
        wall, pas, srt = med('wall_s'), med('pass_ms'), med('sort_ms')
        out[key] = {'all_groups_wall_s': sum(wall), 'all_groups_pass_ms': sum(pas), 'all_groups_sort_ms': sum(srt),
                    'median_group_wall_s': float(np.median(wall)), 'median_group_pass_ms': float(np.median(pas)), 'median_group_sort_ms': float(np.median(srt)),
                    'pass_bytes_per_group': 8 * n_keys,
                    'pass_bytes_per_s': 8 * n_keys / (float(np.median(pas)) * 1e-3) if np.median(pas) > 0 else None,
                    'pass_share_of_copy_ceiling': 8 * n_keys / (float(np.median(pas)) * 1e-3) / COPY_CEILING if np.median(pas) > 0 else None}
    out['per_group_first'] = [{'contigs': r['contigs'], 'edges': r['edges'],
                               **{'bitmap_%d' % k: {what: float(np.median(r['bitmap_%d' % k][what])) for what in ('wall_s', 'pass_ms', 'sort_ms')} for k in knobs}}
                              for r in per_group[:KEEP_GROUPS]]
    out['edges_all_groups'] = int(sum(r['edges'] for r in per_group))
    out['front_total_s'] = out['file_to_table_s'] + out['names_and_ids_s'] + out['bitmap_%d' % knobs[0]]['all_groups_wall_s']
    t0 = clock()
    del table
    gc.collect()
    out['release_s'] = clock() - t0
    return out, kept


def numpy_check(fi, fj, links, names, groups, kept):
    """the kept device results against the numpy restatement of the rule on the same arrays -> the groups compared"""
    from haphic_amd import sort
    from tests import sort_heads_cases as hc
    S = types.SimpleNamespace(get_sub_HT_dict=None)
    _proxy, mirror = sort.bind_heads(S, hc.HostPickle.open)
    table = sort.HTTable(hc.HostPickle.from_arrays(fi, fj, links, names))
    for g in sorted(kept):
        want, _index = mirror(groups[g], table)
        assert all(np.array_equal(x, y) for x, y in zip(kept[g], (want.i, want.j, want.w))), 'group %d differs from the numpy engine' % g
    return sorted(kept)


def parent_front(path, groups, scripts, n_reference_groups, kept):
    """pickle.load, and where the checkout is the reference's get_sub_HT_dict on the first n_reference_groups groups"""
    t0 = clock()
    with open(path, 'rb') as f:
        table = pickle.load(f)
    out = {'pickle_load_s': clock() - t0, 'keys': len(table)}
    if scripts:
        sys.path.insert(0, os.path.join(ROOT))
        from tests import sort_cases as sc
        S = sc.load_reference_sort(scripts, '_haphic_sort_reference_heads_bench')
        out['reference'] = []
        for g, ctgs in enumerate(groups[:n_reference_groups]):
            t0 = clock()
            sub, index = S.get_sub_HT_dict(ctgs, table)
            out['reference'].append({'group': g, 'contigs': len(ctgs), 'edges': len(sub), 'get_sub_HT_dict_s': clock() - t0})
            if g in kept:
                keys = np.array(list(sub.keys()), np.int32).reshape(-1, 2)
                assert np.array_equal(keys[:, 0], kept[g][0]) and np.array_equal(keys[:, 1], kept[g][1]) and list(sub.values()) == kept[g][2].tolist(), g
                out['reference'][-1]['equal_to_the_device_result'] = True
        out['reference_groups_timed'] = len(out['reference'])
        out['reference_all_groups_s'] = sum(r['get_sub_HT_dict_s'] for r in out['reference']) * len(groups) / max(1, len(out['reference']))
        out['reference_all_groups_how'] = 'measured' if len(out['reference']) == len(groups) else 'the timed groups scaled to all (equal-sized groups)'
    t0 = clock()
    del table
    gc.collect()
    out['release_s'] = clock() - t0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--contigs', type=int, default=100000)
    ap.add_argument('--groups', type=int, default=32)
    ap.add_argument('--keys', default='5000000,220000000')
    ap.add_argument('--dict-keys', type=int, default=5000000)
    ap.add_argument('--reference', default=os.environ.get('HAPHIC_REFERENCE'), help="HapHiC's scripts/ directory: time its get_sub_HT_dict too")
    ap.add_argument('--reference-groups', type=int, default=2, help='groups the reference function is timed on (each takes tens of seconds)')
    ap.add_argument('--reference-only', action='store_true', help='no GPU: the parent record at --dict-keys alone (the other records of --out are kept)')
    ap.add_argument('--dir', default=None, help='where the pickles are written (default: a temporary directory)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sort_heads_bench.json'))
    args = ap.parse_args()
    from haphic_amd import _lib
    sizes = [int(k) for k in args.keys.split(',')]
    if args.reference_only:
        sizes = [min(args.dict_keys, max(sizes))]
    group = (np.arange(args.contigs, dtype=np.int64) * args.groups // args.contigs).astype(np.int32)
    names = ['ctg%06d_%s' % (k >> 1, 'HT'[k & 1]) for k in range(2 * args.contigs)]
    groups = groups_of(group, args.groups)
    record = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            record = json.load(f)
    record.update({'contigs': args.contigs, 'groups': args.groups, 'repeats': REPEATS, 'copy_ceiling_bytes_per_s': COPY_CEILING,
                   'yardstick': 'pickle.load on the same file in the same session; the reference\'s get_sub_HT_dict where the checkout exists (see each '
                                'parent record for where it ran)'})
    record.setdefault('sizes', {})
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        for n in sizes:
            fi, fj, links, _group = synth(args.contigs, n, args.groups)       # a table of its own per size: the same in every run
            n = len(fi)
            entry = record['sizes'].setdefault(str(n), {})
            for dialect in ('library', 'python'):
                if dialect == 'python' and n > args.dict_keys:
                    entry['python'] = 'not written: the pickler needs the dict of every key'
                    continue
                path = os.path.join(tmp, '%s_%d.pkl' % (dialect, n))
                if dialect == 'library':
                    _lib.write_link_pickle(path, fi, fj, links, names)
                else:
                    table_names = np.array(names, object)
                    d = defaultdict(int)
                    d.update(zip(zip(table_names[fi].tolist(), table_names[fj].tolist()), links.tolist()))
                    assert len(d) == n
                    with open(path, 'wb') as f:
                        pickle.dump(d, f, 4)
                    del d
                rec = entry.setdefault(dialect, {})
                rec['file_bytes'] = os.path.getsize(path)
                kept = {}
                if not args.reference_only:
                    device_front(path, groups[:2], (1, 0), ())                   # warm: the file in the page cache, pinned buffers
                    rec['device'], kept = device_front(path, groups, (1, 0), set(range(2 if n <= args.dict_keys else 1)))
                    rec['device']['equal_to_the_numpy_engine'] = {'groups': numpy_check(fi, fj, links, names, groups, kept), 'both_knob_settings': True}
                if n <= args.dict_keys:
                    where = 'on the machine with the GPU, same session' if not args.reference_only else 'on a machine without a GPU (same software), its own session'
                    parent = parent_front(path, groups, args.reference if args.reference and os.path.isdir(args.reference) else None, args.reference_groups, kept)
                    parent['where'] = where
                    if args.reference_only:
                        parent['note'] = ('the same table as the device records of this size (same generator, seed and size), another host and session: the '
                                          'times are not comparable row for row with the records taken on the machine with the GPU')
                    rec['parent_reference_only' if args.reference_only else 'parent'] = parent
                os.remove(path)
                print(n, dialect, json.dumps({k: v for k, v in rec.items() if k != 'device'}), flush=True)
                if 'device' in rec:
                    print(n, dialect, json.dumps(rec['device']), flush=True)
                with open(args.out, 'w') as f:                                    # what is measured so far
                    json.dump(record, f, indent=1, sort_keys=True)
        base = record['sizes'].get(str(args.dict_keys), {})
        for n, entry in record['sizes'].items():
            for dialect in ('library',):
                b = base.get(dialect, {}).get('parent')
                if isinstance(entry.get(dialect), dict) and 'parent' not in entry[dialect] and b:
                    entry[dialect]['parent_extrapolated'] = {'pickle_load_s': b['pickle_load_s'] * int(n) / b['keys'], 'from_keys': b['keys'],
                                                             'how': 'by proportion of the keys (pickle.load); get_sub_HT_dict does not depend on the keys: n (n - 1) / 2 pairs x 4 look-ups per group'}
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1, sort_keys=True)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
