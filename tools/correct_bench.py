"""Assembly correction (--correct_nrounds) timed at the BASELINE C3 shape (100 k contigs / 500 M read pairs) on one MI355X, in ONE session on ONE
.pairs file: the synthetic genome and pairs of bench.py (haphic_amd/synth.py) with chimeras planted by synth.join_chimeras.

    (a) pass one from device arrays      _lib.CorrectTable.push_device + finalize on the id / position arrays in HBM, with the plain atomics and
                                         with "correct_agg" (adds merged inside the wave), on the stream as sampled and on a slice grouped by contig
    (b) pass one from the .pairs file    correct.parse_pairs_for_correction: read-ahead reader -> tokeniser -> the same table; then detect_break_points
    (c) pass two to link-matrix-ready    the seam sequence of tools/c3_run.py (stat_fragments ... dict_to_matrix) on the CORRECTED assembly with
                                         pairs_generator_for_correction_ctg (the remap between tokeniser and ingest) — the chimeras cut where they were joined
    (d) the uncorrected run              tools/c3_run.py run_sequence on the same file: text -> link matrix without any correction

(b) and (c) read the same bytes through the same tokeniser as (d): what they cost beyond it is the extra kernels.

    python tools/correct_bench.py [--contigs 100000] [--pairs 500000000] [--chimeras 2000] [--out profiles/correction_bench.json]
    python tools/correct_bench.py --gpus N [--host-transport] [--pairs 20000000] [--out FILE.json]
                                                                                   both passes as N ranks over one .pairs file (haphic_amd/ranks.py):
                                                                                   per rank and per pass the lines parsed, the pairs kept, the seconds
                                                                                   and the bytes sent to rank 0.  Ranks that share a device: functional only
    python tools/correct_bench.py --cpu-reference DIR [--prefix-pairs 200000]     the reference's own parse_pairs_for_correction (CPU, no GPU needed)
                                                                                   on a labelled prefix of such a file; merged into --out
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def pass_one_device(_lib, lens, res, arrays, agg, slice_pairs=1 << 27):
    """-> (seconds, kept pairs, seconds of the finalize alone)"""
    sync = lambda: _lib.check(_lib.load().hhx_synchronize())          # noqa: E731
    _lib.tune('correct_agg', agg)
    try:
        sync()
        t0 = time.perf_counter()
        table = _lib.CorrectTable(lens, res)
        n = arrays[0].numel()
        for lo in range(0, n, slice_pairs):
            hi = min(n, lo + slice_pairs)
            table.push_device(hi - lo, *[t[lo:hi].data_ptr() for t in arrays])
        sync()
        t1 = time.perf_counter()
        kept = table.finalize()
        sync()
        t2 = time.perf_counter()
        table.destroy()
        _lib.check(_lib.load().hhx_pool_trim())
        return t2 - t0, kept, t2 - t1
    finally:
        _lib.tune('correct_agg', None)


def gpu_legs(a):
    import torch
    import c3_run
    from haphic_amd import _lib, cluster, correct, synth
    _lib.check(_lib.load().hhx_set_device(0))
    res = 500
    out = {'what': __doc__.split('\n\n')[1], 'resolution': res, 'device': torch.cuda.get_device_name(0)}
    per_chr = max(1, a.contigs // a.nchrs)
    base = synth.make_genome(a.nchrs, per_chr * a.mean_len, a.mean_len, seed=12345)
    parts = [synth.sample_pairs(base, min(250_000_000, a.pairs - lo), seed=12345 + 1 + 1000 * k, device='cuda:0')
             for k, lo in enumerate(range(0, a.pairs, 250_000_000))]
    arrays = [torch.cat([q[c] for q in parts]) if len(parts) > 1 else parts[0][c] for c in range(4)]
    del parts
    gen, id1, p1, id2, p2, joins = synth.join_chimeras(base, *arrays, a.chimeras, seed=777)
    del arrays
    arrays = [id1.contiguous(), p1.contiguous(), id2.contiguous(), p2.contiguous()]
    del id1, p1, id2, p2
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    names, lens = list(gen.names), gen.length
    out.update(contigs=int(gen.n), pairs=int(arrays[0].numel()), chimeras_planted=len(joins))

    # ---- (a)
    legs = {}
    pass_one_device(_lib, lens, res, [t[:1 << 24] for t in arrays], 0)       # first-launch costs stay out of the figures
    for agg in (0, 1):
        s, kept, fin = pass_one_device(_lib, lens, res, arrays, agg)
        legs['stream_order_agg%d' % agg] = {'seconds': s, 'finalize_s': fin, 'pairs_per_s': arrays[0].numel() / s}
    out['kept_intra_contig_pairs'] = int(kept)
    n_slice = min(arrays[0].numel(), 1 << 26)
    order = torch.sort(arrays[0][:n_slice].long() * 2 + (arrays[0][:n_slice] != arrays[2][:n_slice]).long(), stable=True)[1]
    grouped = [t[:n_slice][order].contiguous() for t in arrays]
    del order
    for agg in (0, 1):
        s, _k, fin = pass_one_device(_lib, lens, res, grouped, agg)
        legs['grouped_by_contig_%d_pairs_agg%d' % (n_slice, agg)] = {'seconds': s, 'finalize_s': fin, 'pairs_per_s': n_slice / s}
    del grouped
    out['a_pass_one_from_device_arrays'] = legs

    # ---- the file (untimed)
    name_bytes = float(np.mean([len(nm) for nm in names]))
    need = a.pairs * ((2 * name_bytes + 30) + (2 * name_bytes + 60) + 56 + 12)
    where = a.dir
    if where is None:
        where = next((c for c in ('/dev/shm', tempfile.gettempdir()) if c3_run.room_for(need, c) is None), None)
    if where is None or c3_run.room_for(need, where) is not None:
        out['skipped_file_legs'] = c3_run.room_for(need, where or '/dev/shm')
        return out
    d = tempfile.mkdtemp(prefix='hhx_correct_bench_', dir=where)
    try:
        path = os.path.join(d, 'hic.pairs')
        size, lines = c3_run.write_pairs_file(path, gen, *arrays)
        del arrays
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        _lib.check(_lib.load().hhx_pool_trim())
        out['pairs_file_bytes'] = int(size)
        sync = lambda: _lib.check(_lib.load().hhx_synchronize())      # noqa: E731

        # ---- (d) first: the figure everything is compared with
        os.makedirs(os.path.join(d, 'plain'))
        plain = c3_run.run_sequence(path, gen, a.nchrs, os.path.join(d, 'plain'), sweep=False)
        shutil.rmtree(os.path.join(d, 'plain'), ignore_errors=True)
        out['d_uncorrected_text_to_link_matrix'] = {'link_matrix_ready_s': plain['seconds']['link_matrix_ready_s'],
                                                    'pairs_text_to_containers_s': plain['seconds']['pairs_text_to_containers_s'],
                                                    'files_join_wait_s': plain['seconds']['files_join_wait_s'], 'matrix_order': plain['matrix_order']}
        _lib.check(_lib.load().hhx_pool_trim())

        # ---- (b)
        fa_dict = {nm: [None, int(ln), int(ln) // 256 + 1] for nm, ln in zip(names, lens.tolist())}
        args = types.SimpleNamespace(alignments=path, aln_format='pairs', correct_resolution=res, median_cov_ratio=0.2, region_len_ratio=0.1,
                                     min_region_cutoff=5000, threads=8)
        sync()
        t0 = time.perf_counter()
        cov_d, pos_d = correct.parse_pairs_for_correction(fa_dict, args)
        sync()
        t1 = time.perf_counter()
        bp = correct.detect_break_points(cov_d, fa_dict, args)
        t2 = time.perf_counter()
        at = {c: k for k, c in enumerate(names)}
        truth = dict(joins)
        hit = sum(1 for c, pts in bp.items() if at[c] in truth and any(abs(p - truth[at[c]]) <= res for p, _v in pts))
        out['b_pass_one_from_pairs_file'] = {'seconds': t1 - t0, 'pairs_per_s': lines / (t1 - t0), 'text_GBs': size / (t1 - t0) / 1e9,
                                             'detect_break_points_s': t2 - t1, 'contigs_with_break_points': len(bp),
                                             'planted_joins_found_within_one_bin': hit}
        del cov_d, pos_d
        _lib.check(_lib.load().hhx_pool_trim())

        # ---- (c): the assembly corrected at the planted joins (the final_break_* dicts in the shape break_and_update_ctgs leaves them)
        fpos, ffrag, cnames, clens = {}, {}, [], []
        for k, (nm, ln) in enumerate(zip(names, lens.tolist())):
            if k in truth:
                cut = truth[k]
                kids = ['{}:1-{}'.format(nm, cut), '{}:{}-{}'.format(nm, cut + 1, ln)]
                fpos[nm], ffrag[nm] = [cut, 0], kids[::-1]
            else:
                cnames.append(nm)
                clens.append(ln)
        for nm in fpos:                                               # children go behind the unbroken contigs, as in fa_dict
            cut = fpos[nm][0]
            total = int(lens[at[nm]])
            cnames += ffrag[nm][::-1]
            clens += [cut, total - cut]
        corrected = types.SimpleNamespace(names=cnames, length=np.asarray(clens, np.int64))
        real = cluster.pairs_generator_inter_ctgs
        cluster.pairs_generator_inter_ctgs = lambda p, fmt: correct.pairs_generator_for_correction_ctg(p, fmt, fpos, ffrag)
        try:
            os.makedirs(os.path.join(d, 'corrected'))
            fixed = c3_run.run_sequence(path, corrected, a.nchrs, os.path.join(d, 'corrected'), sweep=False)
        finally:
            cluster.pairs_generator_inter_ctgs = real
        out['c_pass_two_with_remap_to_link_matrix'] = {'link_matrix_ready_s': fixed['seconds']['link_matrix_ready_s'],
                                                       'pairs_text_to_containers_s': fixed['seconds']['pairs_text_to_containers_s'],
                                                       'files_join_wait_s': fixed['seconds']['files_join_wait_s'], 'matrix_order': fixed['matrix_order'],
                                                       'corrected_contigs': len(cnames)}
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def _planted_correction(names, lens, joins):
    """the final_break_* dicts and the corrected contig table of an assembly cut at the planted joins, in the shape break_and_update_ctgs leaves them"""
    truth = dict(joins)
    fpos, ffrag, cnames, clens = {}, {}, [], []
    for k, (nm, ln) in enumerate(zip(names, lens)):
        if k in truth:
            cut = truth[k]
            fpos[nm], ffrag[nm] = [cut, 0], ['{}:{}-{}'.format(nm, cut + 1, ln), '{}:1-{}'.format(nm, cut)]
        else:
            cnames.append(nm)
            clens.append(ln)
    for k, (nm, ln) in enumerate(zip(names, lens)):
        if k in truth:
            cnames += ffrag[nm][::-1]
            clens += [truth[k], ln - truth[k]]
    return fpos, ffrag, cnames, clens


def ranks_job(meta_path):
    """one rank of the --gpus N mode (started by ranks.launch): rank 0 drives pass one and pass two, the others serve"""
    from haphic_amd import _lib, cluster, correct, ranks
    with open(meta_path) as f:
        meta = json.load(f)
    ctx = ranks.init(True if meta['host_transport'] else None)
    if ctx is None:
        _lib.check(_lib.load().hhx_set_device(0))

    def drive():
        names, lens = meta['names'], meta['lens']
        fa_dict = {nm: [None, int(ln), int(ln) // 256 + 1] for nm, ln in zip(names, lens)}
        args = types.SimpleNamespace(alignments=meta['pairs'], aln_format='pairs', correct_resolution=500, median_cov_ratio=0.2, region_len_ratio=0.1,
                                     min_region_cutoff=5000, threads=8, flank=500, remove_allelic_links=0, remove_concentrated_links=False,
                                     max_read_pairs=200, nwindows=50, skip_clustering=True)
        os.chdir(meta['workdir'])
        cov_d, pos_d = correct.parse_pairs_for_correction(fa_dict, args)
        found = len(correct.detect_break_points(cov_d, fa_dict, args))
        del cov_d, pos_d
        fpos, ffrag, cnames, clens = _planted_correction(names, lens, meta['joins'])
        fixed = {nm: [None, int(ln), int(ln) // 256 + 1] for nm, ln in zip(cnames, clens)}
        _s, _b, _bs, frag_len_dict, nx, _re, split = cluster.stat_fragments(fixed, 'GATC', {}, set(), nchrs=meta['nchrs'], flank=500, Nx=100, bin_size=-1)
        assert not split
        aln = correct.pairs_generator_for_correction_ctg(meta['pairs'], 'pairs', fpos, ffrag)
        out = cluster.parse_alignments_for_ctgs(aln, fixed, args, frag_len_dict, nx, 'int32', 'int32')
        _lib.check(_lib.load().hhx_synchronize())
        n_full = len(out[0])
        del out
        _lib.files_join()
        with open(os.path.join(meta['workdir'], 'rank0_result.json'), 'w') as f:
            json.dump({'contigs_with_break_points': found, 'full_link_keys': n_full}, f)
    return ranks.run_rank(drive)


def ranks_mode(a):
    """the file made here (one process), then N fresh rank processes over it; their records collected"""
    import torch
    import c3_run
    from haphic_amd import _lib, ranks, synth
    _lib.check(_lib.load().hhx_set_device(0))
    per_chr = max(1, a.contigs // a.nchrs)
    base = synth.make_genome(a.nchrs, per_chr * a.mean_len, a.mean_len, seed=12345)
    arrays = synth.sample_pairs(base, a.pairs, seed=12346, device='cuda:0')
    gen, id1, p1, id2, p2, joins = synth.join_chimeras(base, *arrays, a.chimeras, seed=777)
    d = tempfile.mkdtemp(prefix='hhx_correct_ranks_', dir=a.dir or ('/dev/shm' if os.path.isdir('/dev/shm') else None))
    try:
        path = os.path.join(d, 'hic.pairs')
        size, lines = c3_run.write_pairs_file(path, gen, id1.contiguous(), p1.contiguous(), id2.contiguous(), p2.contiguous())
        del arrays, id1, p1, id2, p2
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        _lib.check(_lib.load().hhx_pool_trim())
        rec = os.path.join(d, 'record')
        os.makedirs(rec)
        os.makedirs(os.path.join(d, 'work'))
        meta = os.path.join(d, 'meta.json')
        with open(meta, 'w') as f:
            json.dump({'pairs': path, 'workdir': os.path.join(d, 'work'), 'names': list(gen.names), 'lens': [int(x) for x in gen.length.tolist()],
                       'joins': [[int(k), int(v)] for k, v in joins], 'nchrs': a.nchrs, 'host_transport': bool(a.host_transport)}, f)
        env = dict(os.environ, HAPHIC_RANKS_RECORD=rec)
        env.pop('MASTER_PORT', None)
        t0 = time.perf_counter()
        rc = ranks.launch(['timeout', '-k', '10', str(a.rank_timeout), sys.executable, os.path.abspath(__file__), '--rank-job', meta], a.gpus,
                          host_transport=a.host_transport, env=env)
        wall = time.perf_counter() - t0
        if rc:
            raise SystemExit('the {}-rank job failed with status {}'.format(a.gpus, rc))
        per_rank = []
        for r in range(a.gpus):
            with open(os.path.join(rec, 'rank%d.json' % r)) as f:
                per_rank.append(json.load(f))
        with open(os.path.join(d, 'work', 'rank0_result.json')) as f:
            result = json.load(f)
        shared = a.gpus > _lib.device_count()
        return {'what': 'both correction passes as %d ranks over one .pairs file (pass one = phase correct_pass1, pass two = phase ingest with the remap)' % a.gpus,
                'label': 'functional: %d ranks SHARE %d device(s) over the host transport — content and order, not speed' % (a.gpus, _lib.device_count())
                if shared or a.host_transport else 'one device per rank',
                'device': torch.cuda.get_device_name(0), 'ranks': a.gpus, 'host_transport': bool(a.host_transport or shared),
                'contigs': int(gen.n), 'pairs': int(a.pairs), 'chimeras_planted': len(joins), 'pairs_file_bytes': int(size), 'pairs_file_lines': int(lines),
                'job_wall_s_with_process_start': wall, 'per_rank': per_rank, **result}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def cpu_reference(a):
    """the reference's parse_pairs_for_correction :1300-1344, as it is, on the first --prefix-pairs lines of a file of the same model"""
    from haphic_amd import synth
    for name, attrs in (('pysam', {'set_verbosity': lambda *x, **k: None, 'AlignmentFile': None}), ('portion', {'closed': None, 'empty': None})):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            sys.modules[name] = m
    sys.path.insert(0, a.cpu_reference)
    import HapHiC_cluster as H
    per_chr = max(1, a.contigs // a.nchrs)
    base = synth.make_genome(a.nchrs, per_chr * a.mean_len, a.mean_len, seed=12345)
    arrays = synth.sample_pairs(base, a.prefix_pairs, seed=12346, device='cpu')
    gen, id1, p1, id2, p2, _j = synth.join_chimeras(base, *arrays, a.chimeras, seed=777)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'prefix.pairs')
        with open(path, 'w') as f:
            f.write('## pairs format v1.0\n')
            for k, (u, x, v, y) in enumerate(zip(id1.tolist(), p1.tolist(), id2.tolist(), p2.tolist())):
                f.write('r%d\t%s\t%d\t%s\t%d\t+\t-\n' % (k, gen.names[u], x + 1, gen.names[v], y + 1))
        fa_dict = {nm: [None, int(ln), 1] for nm, ln in zip(gen.names, gen.length.tolist())}
        args = types.SimpleNamespace(alignments=path, aln_format='pairs', correct_resolution=500)
        t0 = time.perf_counter()
        H.parse_pairs_for_correction(fa_dict, args)          # (its first lines build the 100 k empty coverage arrays: part of the call)
        s = time.perf_counter() - t0
    return {'what': "the reference's own parse_pairs_for_correction on a PREFIX of %d read pairs of the same model (one CPU core of the development "
                    'box, not the GPU host; not extrapolated)' % a.prefix_pairs, 'prefix_pairs': a.prefix_pairs, 'seconds': s,
            'pairs_per_s': a.prefix_pairs / s}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--contigs', type=int, default=100000)
    ap.add_argument('--pairs', type=int, default=None, help='read pairs (default 500 M; 20 M with --gpus)')
    ap.add_argument('--nchrs', type=int, default=24)
    ap.add_argument('--mean-len', type=int, default=30_000)
    ap.add_argument('--chimeras', type=int, default=2000)
    ap.add_argument('--dir', default=None)
    ap.add_argument('--out', default=None, help='JSON file to write / merge into')
    ap.add_argument('--cpu-reference', default=None, help="the reference's scripts directory: time its pass one on a prefix instead of the GPU legs")
    ap.add_argument('--prefix-pairs', type=int, default=200_000)
    ap.add_argument('--gpus', type=int, default=0, help='run both passes as this many ranks and report the per-rank record')
    ap.add_argument('--host-transport', action='store_true')
    ap.add_argument('--rank-timeout', type=int, default=600, help='seconds each rank process may run')
    ap.add_argument('--rank-job', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.rank_job:
        sys.exit(ranks_job(a.rank_job))
    if a.gpus > 8:
        ap.error('--gpus: at most 8 ranks (this process keeps its device open beside them)')
    if a.pairs is None:
        a.pairs = 20_000_000 if a.gpus else 500_000_000
    out = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    if a.gpus:
        out['ranks_%d' % a.gpus] = ranks_mode(a)
    elif a.cpu_reference:
        out['cpu_reference_prefix'] = cpu_reference(a)
    else:
        out.update(gpu_legs(a))
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
