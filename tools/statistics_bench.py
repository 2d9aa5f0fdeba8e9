#!/usr/bin/env python3
"""Measures output_statistics :2279-2478 on the device tables (haphic_amd/statistics.py, csrc/hhx_groupstats.hip) and writes
profiles/statistics_bench.json.  A record, not a gate.

    python tools/statistics_bench.py                      (one MI355X: the C3 shape, 99,878 contigs / 500 M pairs synthesised as tools/c3_run.py does)
    python tools/statistics_bench.py --reference DIR      (no GPU: the reference's own output_statistics on the 1k-contig config, one core; the
                                                           figure is merged into the same JSON under "reference_1k_contigs_cpu")

One session on the GPU: the pairs go through the device ingest, full_link_dict stays frozen, then
  (a) `new`: statistics.output_statistics on it for --sets synthetic partitions (n_groups from about 20 to about 9000, contigs that are neighbours
      on a chromosome share a group, 5 % ungrouped), --repeats times: the whole call, and its split into the device call (with the library's HIP
      events per kernel), the host axes, the text files and the PDFs;
  (b) `yardstick`: cluster.group_link_dict on the same table for the same partitions, i.e. the parse_link_dict seam the reference's function runs on
      when this seam is not bound.  That code is the part of the parent's output_statistics that is this project's; the reference's per-contig loop
      over its result comes on top, so it is a LOWER bound of what the parent pays.  It runs in a child process on host copies of the arrays (the
      fetch is timed apart, once) under a time cap per set; a set that hits the cap is recorded as such.  --yardstick-sets picks how many of the
      sets are tried (spread over the range of n_groups)."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
clock = time.perf_counter


def partitions(gen_chrom, n_sets, lo=20, hi=9000, seed=1):
    """[(label, group id per contig)]: contigs in genome order cut into n_groups runs, 5 % ungrouped"""
    rng = np.random.default_rng(seed)
    n = len(gen_chrom)
    out = []
    for k, g in enumerate(np.unique(np.geomspace(lo, min(hi, max(lo, n // 2)), n_sets).astype(np.int64)).tolist()):
        grp = (np.arange(n, dtype=np.int64) * g // n).astype(np.int32)
        grp[rng.random(n) < 0.05] = -1
        out.append(('%.1f' % (1.1 + 0.1 * k), grp))
    return out


def clusters_of(names, grp):
    order = np.argsort(grp, kind='stable')
    g = grp[order]
    cuts = np.flatnonzero(np.diff(g, prepend=-1)).tolist() + [len(g)]
    table = np.empty(len(names), object)
    table[:] = names
    return [(table[order[a:b]].tolist(), None) for a, b in zip(cuts[:-1], cuts[1:]) if g[a] >= 0]


class HostTable:
    """a frozen full_link_dict over host arrays (the yardstick's child has no handle)"""

    def __init__(self, i, j, v, names):
        self.i, self.j, self.v = i, j, v
        self.table = types.SimpleNamespace(ctg_names=names)

    def n_keys(self, kind):
        return len(self.i)

    def link_arrays(self, kind):
        return self.i, self.j, self.v, self.table.ctg_names

    def note_thawed(self):
        pass


def yardstick_child(path, which):
    from haphic_amd import cluster, containers
    z = np.load(os.path.join(path, 'table.npz'))
    with open(os.path.join(path, 'names.txt')) as f:
        names = f.read().split('\n')
    grp = np.load(os.path.join(path, 'set_%d.npy' % which))
    full = containers.LinkTable(HostTable(z['i'], z['j'], z['v'], names), 'full')
    ctg_group = {n: ('ungrouped' if g < 0 else g) for n, g in zip(names, grp.tolist())}
    t0 = clock()
    out = cluster.group_link_dict(full, ctg_group)
    print(json.dumps({'group_link_dict_s': clock() - t0, 'contigs_with_cells': len(out)}))


def device_run(opt):
    import torch                                             # noqa: F401 (the pairs are sampled on the device)
    from haphic_amd import _lib, build, cluster, containers, statistics, synth
    _lib.check(_lib.load().hhx_set_device(0))
    per_chr = max(1, opt.contigs // opt.nchrs)
    gen = synth.make_genome(opt.nchrs, per_chr * opt.mean_len, opt.mean_len, seed=12345)
    names = list(gen.names)
    rec = {'what': 'output_statistics :2279-2478 for %d partitions of one frozen full_link_dict, one MI355X' % opt.sets, 'source_hash': build.source_hash(),
           'contigs': gen.n, 'pairs': opt.pairs, 'repeats': opt.repeats}
    t0 = clock()
    table = cluster.FragTable.for_contigs(gen.lexical_rank(), gen.length, np.ones(gen.n, np.uint8), names)
    ing = _lib.Ingest(table, 500_000, bins=False, skip_intra=True)
    chunk = 1 << 24
    for k, lo in enumerate(range(0, opt.pairs, chunk)):
        n = min(chunk, opt.pairs - lo)
        id1, p1, id2, p2 = synth.sample_pairs(gen, n, seed=12345 + 1 + 1000 * k, device='cuda:0')
        torch.cuda.synchronize()
        ing.push_device(n, id1.data_ptr(), p1.data_ptr(), id2.data_ptr(), p2.data_ptr())
        _lib.check(_lib.load().hhx_synchronize())
        del id1, p1, id2, p2
    torch.cuda.empty_cache()
    ing.finalize()
    a = types.SimpleNamespace(remove_allelic_links=0, remove_concentrated_links=False, max_read_pairs=0, nwindows=50)
    session = cluster.IngestSession(ing, table, None, a, 'int32', 'int32')
    full = containers.LinkTable(session, 'full')
    rec['ingest_s'] = round(clock() - t0, 2)
    rec['full_keys'] = len(full)
    fa_dict = {nm: [None, int(ln), int(ln) // 256 + 1] for nm, ln in zip(names, gen.length.tolist())}
    sets = partitions(gen.chrom, opt.sets)
    rcl = [(label, clusters_of(names, grp)) for label, grp in sets]
    rec['n_groups'] = [len(c) for _l, c in rcl]
    work = tempfile.mkdtemp(prefix='hhx_stats_', dir=opt.dir)
    cwd = os.getcwd()
    try:
        os.chdir(work)
        for label, _c in rcl:
            os.makedirs('inflation_' + label)
        # ---- (a) the mirrored call
        runs = []
        for r in range(opt.repeats):
            del containers.THAW_LOG[:]
            _lib.profile_reset()
            _lib.profile_enable(True)
            t0 = clock()
            statistics.output_statistics(fa_dict, full, rcl)
            wall = clock() - t0
            _lib.profile_enable(False)
            assert full.frozen and not containers.THAW_LOG and statistics.STATS['engine'] == 'device'
            st = statistics.STATS
            runs.append({'wall_s': round(wall, 3), 'device_call_s': round(st['device_s'], 3), 'host_axes_s': round(st['axes_s'], 3),
                         'text_files_s': round(st['text_s'], 3), 'pdf_s': round(st['pdf_s'], 3),
                         'kernels_ms': {k: round(_lib.profile_get(k)[0], 2) for k in ('groupstats_adjacency', 'groupstats_rows', 'groupstats_spill')},
                         'rows_spilled': _lib.profile_counter('groupstats_spilled')})
            print('new', r, json.dumps(runs[-1]), flush=True)
        rec['new'] = {'runs': runs, 'wall_s_min_max': [min(x['wall_s'] for x in runs), max(x['wall_s'] for x in runs)],
                      'text_bytes': sum(os.path.getsize(os.path.join(d, f)) for d in os.listdir('.') for f in os.listdir(d) if f.endswith('.txt'))}
        # ---- (b) the yardstick: group_link_dict per set on host copies, in a child under a time cap
        if opt.yardstick_sets:
            t0 = clock()
            i, j, v, _names = full.arrays()
            fetch_s = clock() - t0
            np.savez(os.path.join(work, 'table.npz'), i=i, j=j, v=v)
            with open(os.path.join(work, 'names.txt'), 'w') as f:
                f.write('\n'.join(names))
            picks = sorted(set(np.linspace(0, len(sets) - 1, opt.yardstick_sets).astype(int).tolist()))
            ys = []
            for which in picks:
                np.save(os.path.join(work, 'set_%d.npy' % which), sets[which][1])
                t0 = clock()
                item = {'set': which, 'n_groups': rec['n_groups'][which]}
                try:
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), '--yardstick-child', work, '--which', str(which)], capture_output=True,
                                       text=True, timeout=opt.cap, cwd=ROOT)
                    if p.returncode == 0:
                        item.update(json.loads(p.stdout.strip().split('\n')[-1]))
                    else:
                        item['failed'] = p.stderr[-300:]
                except subprocess.TimeoutExpired:
                    item['hit_the_cap_of_s'] = opt.cap
                item['child_wall_s'] = round(clock() - t0, 2)
                ys.append(item)
                print('yardstick', json.dumps(item), flush=True)
            rec['yardstick'] = {'what': 'cluster.group_link_dict (the parse_link_dict seam) per set, host arrays, child process; a lower bound of the parent\'s '
                                        'output_statistics: the reference\'s per-contig loop over the dict comes on top', 'fetch_table_to_host_s': round(fetch_s, 2),
                                'sets_tried': len(picks), 'of': len(sets), 'per_set': ys}
    finally:
        os.chdir(cwd)
        shutil.rmtree(work, ignore_errors=True)
        session.ing = None
        ing.destroy()
    return rec


def reference_run(opt):
    """(c) the reference's own function on the 1k-contig config (BASELINE.json configs[0]: 4 chromosomes, 1 M pairs), this machine's CPU, one core"""
    for name, attrs in (('pysam', {'set_verbosity': lambda *a, **k: None, 'AlignmentFile': None}), ('portion', {'closed': None, 'empty': None})):
        try:
            __import__(name)
        except ImportError:
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            sys.modules[name] = m
    scripts = opt.reference if os.path.isfile(os.path.join(opt.reference, 'HapHiC_cluster.py')) else os.path.join(opt.reference, 'scripts')
    sys.path.insert(0, scripts)
    import HapHiC_cluster as H
    from haphic_amd import synth
    H.logger.setLevel('WARNING')
    gen = synth.make_genome(4, 25_000_000, 100_000, cv=0.3, min_len=5000, seed=12345)
    names = list(gen.names)
    id1, _p1, id2, _p2 = [t.numpy().astype(np.int64) for t in synth.sample_pairs(gen, 1_000_000, seed=12345)]
    rank = gen.lexical_rank().astype(np.int64)
    swap = rank[id1] > rank[id2]
    a, b = np.where(swap, id2, id1), np.where(swap, id1, id2)
    keep = a != b
    key, first, cnt = np.unique(a[keep] * gen.n + b[keep], return_index=True, return_counts=True)
    order = np.argsort(first, kind='stable')
    link_dict = {(names[k // gen.n], names[k % gen.n]): int(c) for k, c in zip(key[order].tolist(), cnt[order].tolist())}
    fa_dict = {nm: [None, int(ln), int(ln) // 256 + 1] for nm, ln in zip(names, gen.length.tolist())}
    sets = partitions(gen.chrom, opt.sets, lo=4, hi=400)
    rcl = [(label, clusters_of(names, grp)) for label, grp in sets]
    work = tempfile.mkdtemp(prefix='hhx_stats_ref_')
    cwd = os.getcwd()
    try:
        os.chdir(work)
        for label, _c in rcl:
            os.makedirs('inflation_' + label)
        t0 = clock()
        H.output_statistics(fa_dict, link_dict, rcl)
        wall = clock() - t0
    finally:
        os.chdir(cwd)
        shutil.rmtree(work, ignore_errors=True)
    return {'what': 'the unmodified reference\'s output_statistics on a plain dict, 1k-contig config, development box CPU, one core, PDFs included; NOT the GPU box',
            'contigs': gen.n, 'pairs': 1_000_000, 'keys': len(link_dict), 'sets': len(rcl), 'n_groups': [len(c) for _l, c in rcl], 'wall_s': round(wall, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'statistics_bench.json'))
    ap.add_argument('--contigs', type=int, default=100000)
    ap.add_argument('--pairs', type=int, default=500_000_000)
    ap.add_argument('--nchrs', type=int, default=24)
    ap.add_argument('--mean-len', type=int, default=30_000)
    ap.add_argument('--sets', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--yardstick-sets', type=int, default=20)
    ap.add_argument('--cap', type=float, default=600.0, help='seconds one set of the yardstick may take')
    ap.add_argument('--dir', default=None)
    ap.add_argument('--reference', default=None, help='the HapHiC checkout: run (c) here instead of the GPU legs')
    ap.add_argument('--yardstick-child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--which', type=int, default=0, help=argparse.SUPPRESS)
    opt = ap.parse_args()
    if opt.yardstick_child:
        return yardstick_child(opt.yardstick_child, opt.which)
    rec = {}
    if os.path.exists(opt.out):
        with open(opt.out) as f:
            rec = json.load(f)
    if opt.reference:
        rec['reference_1k_contigs_cpu'] = reference_run(opt)
    else:
        keep = rec.get('reference_1k_contigs_cpu')
        rec = device_run(opt)
        if keep:
            rec['reference_1k_contigs_cpu'] = keep
    print(json.dumps(rec, indent=1))
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
