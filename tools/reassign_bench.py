#!/usr/bin/env python3
"""Measures the rounds of `haphic reassign` on the device (haphic_amd/reassign.py, csrc/hhx_reassign.hip) and writes
profiles/reassign_bench.json.  A record, not a gate.

    python tools/reassign_bench.py                     (one MI355X: the C3 shape, 100,000 contigs / 1.65e8 keys of full_link_dict, synthetic)
    python tools/reassign_bench.py --reference DIR     (no GPU: the reference's own parse_link_dict, run_reassignment and
                                                        agglomerative_hierarchical_clustering on the same contigs with --dict-keys keys, one core;
                                                        merged into the same JSON under "reference_cpu")

The job: contigs in --groups planted groups, every contig with keys mostly inside its group; 15 % of the contigs start ungrouped and 15 % in a
wrong group ("planted"), or 80 % start ungrouped ("most_move": the worst case for the launch count, one launch pair per mover).
On the GPU, per grouping:
  (a) the library on arrays at the full shape: hhx_reassign_create (wall), five rounds and the rescue round, stopping at convergence as run()
      :865-880 does (per call: movers, launch pairs, device time by the library's HIP events, wall), hhx_reassign_pair_sums (wall);
  (b) the seams on a real Python dict, for the same contigs with --dict-keys keys (a dict of all 1.65e8 keys takes tens of GB and minutes to
      build, which is the cost this step keeps: "dict_build_s" is that cost at --dict-keys): parse_link_dict of patch_reassign(R, rounds=True)
      and the first round through the mirror, and parse_link_dict of the parent's binding (cluster.parse_link_dict: device sums, then the
      nested dicts and the linked-contig sets rebuilt key by key).
The parent's rounds and agglomerative step are the reference's own loops and need its checkout: the --reference mode times them on the same
smaller job."""
import argparse
import json
import logging
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
clock = time.perf_counter
PARAMS = dict(min_RE_sites=25, min_links=25, min_link_density=0.0001, min_density_ratio=4, ambiguous_cutoff=0.6, max_ctg_len=10000)


_KEYS = {}


def synth_keys(n_ctg, n_keys, n_groups, seed):
    """the keys and links alone (shared by the groupings of one shape)"""
    if (n_ctg, n_keys, n_groups, seed) in _KEYS:
        return _KEYS[(n_ctg, n_keys, n_groups, seed)]
    rng = np.random.default_rng(seed)
    true = (np.arange(n_ctg, dtype=np.int64) * n_groups // n_ctg).astype(np.int32)
    per = n_ctg // n_groups
    m = int(n_keys * 1.15)
    a = rng.integers(0, n_ctg, m)
    inside = rng.random(m) < 0.8
    b = np.where(inside, np.minimum(n_ctg - 1, true[a].astype(np.int64) * per + rng.integers(0, per, m)), rng.integers(0, n_ctg, m))
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = np.unique((lo * n_ctg + hi)[lo != hi])
    del a, b, lo, hi, inside
    key = key[rng.permutation(key.size)[:n_keys]]
    fi, fj = (key // n_ctg).astype(np.int32), (key % n_ctg).astype(np.int32)
    links = np.where(true[fi] == true[fj], rng.integers(5, 60, fi.size), rng.integers(1, 10, fi.size)).astype(np.int64)
    _KEYS.clear()
    _KEYS[(n_ctg, n_keys, n_groups, seed)] = (true, fi, fj, links)
    return true, fi, fj, links


def synth(n_ctg, n_keys, n_groups, ungrouped, wrong, seed=3):
    true, fi, fj, links = synth_keys(n_ctg, n_keys, n_groups, seed)
    rng = np.random.default_rng(seed + 1)
    group = true.copy()
    u = rng.random(n_ctg)
    group[u < ungrouped] = -1
    w = (u >= ungrouped) & (u < ungrouped + wrong)
    group[w] = rng.integers(0, n_groups, int(w.sum()))
    ctg_re = rng.integers(30, 400, n_ctg).astype(np.int64)
    ctg_len = ctg_re * 400
    group_re = np.ones(n_groups, np.int64)
    np.add.at(group_re, group[group >= 0], ctg_re[group >= 0] - 1)
    return dict(fi=fi, fj=fj, links=links, group=group, group_re=group_re, ctg_re=ctg_re, ctg_len=ctg_len,
                order=np.argsort(-ctg_len, kind='stable').astype(np.int32), n_groups=n_groups)


def library_phases(job):
    from haphic_amd import _lib, statistics
    n_ctg = len(job['group'])
    t0 = clock()
    engine = _lib.Reassign(job['fi'], job['fj'], job['links'], n_ctg, job['group'], job['n_groups'])
    out = {'create_wall_s': clock() - t0, 'calls': []}
    group, group_re = job['group'].copy(), job['group_re'].copy()
    flags = ((job['ctg_re'] - 1 >= PARAMS['min_RE_sites']).astype(np.uint8) | ((job['ctg_len'] <= PARAMS['max_ctg_len'] * 1000).astype(np.uint8) << 1))
    _lib.profile_enable(True)

    def call(nround):
        _lib.profile_reset()
        t0 = clock()
        counts = engine.round(group, group_re, job['ctg_re'], job['order'], flags, None, PARAMS['min_links'], PARAMS['min_link_density'],
                              PARAMS['min_density_ratio'], PARAMS['ambiguous_cutoff'], nround == 0, False, statistics.SUM_MODE)
        wall = clock() - t0
        out['calls'].append({'nround': nround, 'counts': counts.tolist(), 'movers': int(counts[1] + counts[2]), 'launch_pairs': engine.launches,
                             'device_ms': _lib.profile_get('reassign_round')[0], 'wall_s': wall})
    last = None
    for n in range(5):                                                   # run() :865-880
        call(n + 1)
        if n > 0 and (last == group).all():
            out['calls'][-1]['converged'] = True
            break
        last = group.copy()
    call(0)
    _lib.profile_enable(False)
    member = (job['group'] >= 0).astype(np.uint8)
    t0 = clock()
    sums, first = engine.pair_sums(member, group, job['n_groups'])
    out['pair_sums_wall_s'] = clock() - t0
    out['pair_cells'] = int((first >= 0).sum())
    out['rounds_wall_s'] = sum(c['wall_s'] for c in out['calls'])
    engine.close()
    return out


def prefix_dicts(job, n_dict_keys):
    n_ctg = len(job['group'])
    names = ['ctg%06d' % k for k in range(n_ctg)]
    k = min(n_dict_keys, len(job['fi']))
    t0 = clock()
    table = np.empty(n_ctg, object)
    table[:] = names
    link_dict = dict(zip(zip(table[job['fi'][:k]].tolist(), table[job['fj'][:k]].tolist()), job['links'][:k].tolist()))
    build = clock() - t0
    gnames = ['group%d' % g for g in range(job['n_groups'])]
    ctg_group_dict = {names[c]: (gnames[g] if g >= 0 else 'ungrouped') for c, g in enumerate(job['group'].tolist())}
    return names, gnames, link_dict, ctg_group_dict, build


def seam_phases(job, n_dict_keys):
    from haphic_amd import cluster, patch
    names, gnames, link_dict, ctg_group_dict, build = prefix_dicts(job, n_dict_keys)
    R = types.ModuleType('HapHiC_reassign_stand_in')
    R.logger = logging.getLogger('reassign_bench')
    for name in ('parse_link_dict', 'run_reassignment', 'agglomerative_hierarchical_clustering', 'split_clm_file'):
        setattr(R, name, None)
    patch.patch_reassign(R, rounds=True)
    out = {'dict_keys': len(link_dict), 'dict_build_s': build}
    t0 = clock()
    tables = R.parse_link_dict(link_dict, ctg_group_dict)
    out['parse_link_dict_rounds_s'] = clock() - t0
    out['tables'] = type(tables[0]).__name__
    t0 = clock()
    rc = R.run_reassignment([(names[c], int(job['ctg_len'][c])) for c in job['order'].tolist()], tables[0], ctg_group_dict, link_dict, tables[1],
                            None, dict(zip(names, job['ctg_re'].tolist())), None, dict(zip(gnames, job['group_re'].tolist())), PARAMS['max_ctg_len'],
                            PARAMS['min_RE_sites'], PARAMS['min_links'], PARAMS['min_link_density'], PARAMS['min_density_ratio'],
                            PARAMS['ambiguous_cutoff'], 0, set(), 1)
    assert rc is None
    out['run_reassignment_round1_mirror_s'] = clock() - t0
    del tables
    names, gnames, link_dict, ctg_group_dict, _ = prefix_dicts(job, n_dict_keys)
    t0 = clock()
    cluster.parse_link_dict(link_dict, ctg_group_dict)
    out['parse_link_dict_parent_s'] = clock() - t0
    return out


def reference_phases(job, n_dict_keys, scripts):
    for name, attrs in (('pysam', {'set_verbosity': lambda *a, **k: None, 'AlignmentFile': None}), ('portion', {'closed': None, 'empty': None})):
        try:
            __import__(name)
        except ImportError:
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            sys.modules[name] = m
    sys.path.insert(0, scripts)
    import HapHiC_reassign as R
    R.logger.setLevel(logging.WARNING)
    names, gnames, link_dict, ctg_group_dict, build = prefix_dicts(job, n_dict_keys)
    out = {'dict_keys': len(link_dict), 'dict_build_s': build, 'calls': []}
    t0 = clock()
    cgl, linked = R.parse_link_dict(link_dict, ctg_group_dict)
    out['parse_link_dict_s'] = clock() - t0
    fa_dict = {names[c]: [None, int(job['ctg_len'][c]), int(job['ctg_re'][c])] for c in range(len(names))}
    RE_site_dict = dict(zip(names, job['ctg_re'].tolist()))
    group_RE_dict = dict(zip(gnames, job['group_re'].tolist()))
    sorted_ctg_list = [(names[c], int(job['ctg_len'][c])) for c in job['order'].tolist()]
    last = None
    for n in range(5):
        before = dict(ctg_group_dict)
        t0 = clock()
        R.run_reassignment(sorted_ctg_list, cgl, ctg_group_dict, link_dict, linked, fa_dict, RE_site_dict, None, group_RE_dict, PARAMS['max_ctg_len'],
                           PARAMS['min_RE_sites'], PARAMS['min_links'], PARAMS['min_link_density'], PARAMS['min_density_ratio'],
                           PARAMS['ambiguous_cutoff'], 0, set(), n + 1)
        out['calls'].append({'nround': n + 1, 'wall_s': clock() - t0, 'movers': sum(1 for c in before if before[c] != ctg_group_dict[c])})
        if n > 0 and last == ctg_group_dict:
            break
        last = ctg_group_dict.copy()
    t0 = clock()
    R.run_reassignment(sorted_ctg_list, cgl, ctg_group_dict, link_dict, linked, fa_dict, RE_site_dict, None, group_RE_dict, PARAMS['max_ctg_len'],
                       PARAMS['min_RE_sites'], PARAMS['min_links'], PARAMS['min_link_density'], PARAMS['min_density_ratio'], PARAMS['ambiguous_cutoff'],
                       0, set(), 0)
    out['calls'].append({'nround': 0, 'wall_s': clock() - t0})
    out['rounds_wall_s'] = sum(c['wall_s'] for c in out['calls'])
    # :494-508 alone (the loop the pair sums replace); the clustering of a few dozen groups behind it is the same code on both sides
    grouped = {c for c, g in ctg_group_dict.items() if g != 'ungrouped'}
    t0 = clock()
    pair = {}
    for (a, b), v in link_dict.items():
        if a not in grouped or b not in grouped:
            continue
        if a not in ctg_group_dict or b not in ctg_group_dict:
            continue
        ga, gb = ctg_group_dict[a], ctg_group_dict[b]
        if ga == gb:
            continue
        k = tuple(sorted([ga, gb]))
        pair[k] = pair.get(k, 0) + v
    out['pair_sums_loop_s'] = clock() - t0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--contigs', type=int, default=100000)
    ap.add_argument('--keys', type=int, default=165000000)
    ap.add_argument('--groups', type=int, default=32)
    ap.add_argument('--dict-keys', type=int, default=5000000)
    ap.add_argument('--reference', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'reassign_bench.json'))
    args = ap.parse_args()
    record = json.load(open(args.out)) if os.path.exists(args.out) else {}
    shape = {'contigs': args.contigs, 'keys': args.keys, 'groups': args.groups, 'dict_keys': args.dict_keys, 'params': PARAMS}
    if args.reference:
        scripts = args.reference if os.path.isfile(os.path.join(args.reference, 'HapHiC_reassign.py')) else os.path.join(args.reference, 'scripts')
        job = synth(args.contigs, args.dict_keys, args.groups, 0.15, 0.15)      # the prefix is all this mode needs
        record['reference_cpu'] = dict(shape=dict(shape, keys=args.dict_keys), note='the reference\'s own functions on the dict of --dict-keys keys, one core, no GPU',
                                       planted=reference_phases(job, args.dict_keys, scripts))
    else:
        record['shape'] = shape
        from haphic_amd import _lib
        _lib.Reassign(np.zeros(1, np.int32), np.ones(1, np.int32), np.ones(1, np.int64), 2, np.zeros(2, np.int32), 1).close()   # the device is up before anything is timed
        for label, ungrouped, wrong in (('planted', 0.15, 0.15), ('most_move', 0.8, 0.0)):
            t0 = clock()
            job = synth(args.contigs, args.keys, args.groups, ungrouped, wrong)
            record[label] = {'synth_s': clock() - t0, 'keys': int(len(job['fi'])), 'library': library_phases(job)}
            print(label, json.dumps(record[label]['library']), flush=True)
            if label == 'planted':
                small = synth(args.contigs, args.dict_keys, args.groups, ungrouped, wrong)
                record[label]['seams_on_dict_prefix'] = seam_phases(small, args.dict_keys)
                print(label, json.dumps(record[label]['seams_on_dict_prefix']), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
