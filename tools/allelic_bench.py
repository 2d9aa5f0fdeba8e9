#!/usr/bin/env python3
"""Measures --remove_allelic_links on the device tables (haphic_amd/allelic.py, csrc/hhx_allelic.hip) on BASELINE.json configs[3] at its stated
size — the 40k-contig autotetraploid of tests/c4_40k.inputs(), 20 M read pairs — and writes profiles/allelic_bench.json.  A record, not a gate.

    python tools/allelic_bench.py [--out profiles/allelic_bench.json]
    python tools/allelic_bench.py --engine oracle        (no GPU: the host half alone, with the numpy engine of tests/allelic_cases.py; nothing is written)

One session: the S5 mirror ingests the pairs, then
  * `stage2_host`, `device`: allelic.remove_allelic_HiC_links on the frozen containers, once with stage 2 as host numpy + scipy (HAPHIC_ALLELIC_STAGE2=host)
    and once with hhx_allelic_nonmax (=device), each on its own ingest — the wall from "filter_fragments returned" to "remaining_frags returned",
    split into the concordance call (its kernel by HIP events, and the 8 B per kept coordinate pair it must read over that time), the allele groups
    (networkx), stage 2 (which form ran, candidates, unique group pairs, how many of them need an assignment solved, seconds inside scipy's loop or
    the device time of hhx_allelic_nonmax by HIP events) and hhx_ingest_drop_links;
  * `parent`: what the same call costs before the reference's loops even start when the seam is not bound — the thaw of full_link_dict,
    flank_link_dict and ctg_coord_dict (containers.THAW_LOG), measured on a second ingest of the same pairs.
The verdict is compared with tests/golden/pipeline_c4_40k.npz (the reference's own run) when that file is present.  Needs networkx."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import c4_40k      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'allelic_bench.json'))
    ap.add_argument('--engine', choices=('device', 'oracle'), default='device')
    ap.add_argument('--skip-parent', action='store_true', help='do not measure the thaw of the three containers')
    opt = ap.parse_args()
    from haphic_amd import allelic, build, cluster, containers
    if opt.engine == 'oracle':
        import haphic_amd
        from tests import allelic_cases
        cluster._lib = haphic_amd._lib = allelic_cases.library()
    from haphic_amd import _lib
    clock = time.perf_counter
    cfg = c4_40k.CFG
    t0 = clock()
    gen, _base, id1, p1, id2, p2 = c4_40k.inputs()
    names = list(gen.names)
    fa_dict = {n: [None, int(l), int(r)] for n, l, r in zip(names, gen.length, gen.re_sites)}
    frag_len_dict = {n: fa_dict[n][1] for n in names}
    args = types.SimpleNamespace(flank=cfg['flank'], remove_allelic_links=cfg['ploidy'], remove_concentrated_links=False, max_read_pairs=cfg['max_read_pairs'],
                                 min_read_pairs=cfg['min_read_pairs'], concordance_ratio_cutoff=cfg['concordance_ratio_cutoff'], nwindows=cfg['nwindows'],
                                 ul=None, skip_clustering=True)
    rec = {'what': 'remove_allelic_HiC_links :474-692 on C4 at 40k contigs', 'engine': opt.engine, 'source_hash': build.source_hash(),
           'contigs': len(names), 'pairs': int(len(id1)), 'inputs_s': round(clock() - t0, 2)}

    def ingest():
        return cluster.parse_alignments_for_ctgs(cluster.IdArrays(names, id1, p1, id2, p2), fa_dict, args, frag_len_dict, set(names), 'int32', 'int32')
    profiling = opt.engine == 'device'
    # ---- the call, once per form of stage 2 (on a fresh ingest each: the call drops links from the tables); the last one is what the verdict is checked on
    for stage2 in (['host', 'device'] if opt.engine == 'device' else ['host']):
        os.environ['HAPHIC_ALLELIC_STAGE2'] = stage2
        t0 = clock()
        full, flank, _ht, _clm, _fl, coord = ingest()
        del _ht, _clm
        rec['ingest_s'] = round(clock() - t0, 2)
        rec['keys'] = {'full': len(full), 'flank': len(flank)}
        pre_full, pre_flank = full.arrays()[:2], flank.arrays()[:2]
        cnt = full.arrays()[2]
        kept_pairs = int(np.minimum(cnt, cfg['max_read_pairs']).sum())
        all_pairs = int(cnt.sum())
        filtered = set(names)
        del containers.THAW_LOG[:]
        if profiling:
            _lib.profile_reset()
            _lib.profile_enable(True)
        t0 = clock()
        remaining = allelic.remove_allelic_HiC_links(fa_dict, coord, full, args, flank, filtered)
        wall = clock() - t0
        assert not containers.THAW_LOG, 'the array path was not taken'
        st = dict(allelic.STATS)
        assert st['stage2_engine'] == stage2, st['stage2_engine']
        dev = {'stage2_engine': st['stage2_engine'], 'wall_s': round(wall, 3), 'total_s': round(st['total_s'], 3), 'concordance_call_s': round(st['concordance_s'], 3),
               'allele_groups_s': round(st['groups_s'], 3),
               'stage2_s': round(st['stage2_s'], 3), 'stage2_candidates': st['candidates'], 'stage2_group_pairs': st['group_pairs'], 'stage2_assignments': st['assignments'],
               'linear_sum_assignment_s': round(st['assignment_s'], 3), 'drop_links_call_s': round(st['drop_s'], 3),
               'stage1_keys': st['stage1_keys'], 'stage2_keys': st['stage2_keys'], 'allele_groups': st['allele_groups'], 'fragments_kept': len(remaining)}
        if profiling:
            _lib.profile_enable(False)
            ms = _lib.profile_get('concordance')[0]
            dev['concordance_kernels_ms'] = round(ms, 3)
            dev['drop_links_device_ms'] = round(_lib.profile_get('drop_links')[0], 3)
            if stage2 == 'device':
                # HIP events around hhx_allelic_nonmax's kernels, scans and sort (its host-to-device copies of the keys are outside them)
                dev['allelic_nonmax_device_ms'] = round(_lib.profile_get('allelic_nonmax')[0], 3)
            dev['kept_coordinate_pairs'] = kept_pairs
            # the kernels read the first min(count, max_read_pairs) records of 8 B of every key; the grouping before them sorts all records
            dev['concordance_GBps_of_needed_bytes'] = round(8 * kept_pairs / (ms * 1e-3) / 1e9, 2) if ms else None
            dev['grouped_records'] = all_pairs
        rec['device' if stage2 == 'device' or opt.engine == 'oracle' else 'stage2_host'] = dev
        if stage2 != 'device' and opt.engine == 'device':
            del full, flank, coord
    # ---- against the reference's own run
    path = os.path.join(ROOT, 'tests', 'golden', 'pipeline_c4_40k.npz')
    if os.path.exists(path):
        g = np.load(path)
        if c4_40k.checksum(id1, p1, id2, p2) == int(g['pairs_checksum']):
            n = len(names)
            key = lambda i, j: i.astype(np.int64) * n + j                                                  # noqa: E731
            fi, fj = full.arrays()[:2]
            ki, kj = flank.arrays()[:2]
            full_removed = ~np.isin(key(*pre_full), key(fi, fj))
            flank_removed = ~np.isin(key(*pre_flank), key(ki, kj))
            want_full = np.unpackbits(g['full_removed'])[:len(full_removed)].astype(bool)
            want_flank = np.unpackbits(g['flank_removed'])[:len(flank_removed)].astype(bool)
            same = bool(np.array_equal(full_removed, want_full) and np.array_equal(flank_removed, want_flank) and
                        [f in remaining for f in names] == g['remaining'].astype(bool).tolist())
            rec['verdict_equals_reference'] = same
            rec['full_removed'], rec['flank_removed'] = int(full_removed.sum()), int(flank_removed.sum())
            assert same, 'the verdict differs from tests/golden/pipeline_c4_40k.npz'
        else:
            rec['verdict_equals_reference'] = 'not compared: the torch CPU generator differs from the one that made the fixture'
    # ---- the parent's floor: thawing the three containers
    if not opt.skip_parent:
        del full, flank, coord
        full, flank, _ht, _clm, _fl, coord = ingest()
        del _ht, _clm, containers.THAW_LOG[:]
        t0 = clock()
        for d in (coord, full, flank):
            d._thaw()
        rec['parent'] = {'thaw_wall_s': round(clock() - t0, 2), 'thaw': {kind: {'keys': keys, 's': round(sec, 2)} for kind, keys, sec in containers.THAW_LOG},
                         'note': 'before the reference\'s per-key loops (:579-599, :634-667) start; they are not measured here'}
    print(json.dumps(rec, indent=1))
    if opt.engine == 'device':
        os.makedirs(os.path.dirname(opt.out), exist_ok=True)
        with open(opt.out, 'w') as f:
            json.dump(rec, f, indent=1)
            f.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
