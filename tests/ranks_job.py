"""One rank of a multi-rank `haphic cluster` job over a .pairs file, for tests/test_gpu_ranks_job.py: run()'s seam sequence (:2829-2945, as
tools/c3_run.run_sequence drives it) on rank 0, ranks.serve() on the others.  Started by ranks.launch() with RANK / WORLD_SIZE set:

    python tests/ranks_job.py CASE PAIRS FORMAT WORKDIR        CASE: toy | bins | bins_allelic | c1 (the fixtures of tests/golden)

HAPHIC_TEXT_CHUNK_MB (read when haphic_amd.cluster is imported) sets the reader's chunk: the tests give the multi-rank runs small chunks, so
that a rank's share is cut into several pushes where the one-rank run makes one."""
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class Args:
    flank = 500
    remove_allelic_links = 0
    remove_concentrated_links = False
    max_read_pairs = 200
    nwindows = 50
    skip_clustering = False


def c1_genome():
    """BASELINE.json configs[0] as tests/test_gpu_pipeline.py makes it: ~1k contigs, 1 M read pairs (the inter-contig ones kept), nchrs 4"""
    from haphic_amd import synth
    gen = synth.make_genome(4, 25_000_000, 100_000, cv=0.3, min_len=5000, seed=12345)
    id1, p1, id2, p2 = [t.numpy() for t in synth.sample_pairs(gen, 1_000_000, seed=12345)]
    return gen, (id1, p1, id2, p2)


def fixture(case):
    from tests.conftest import load_golden
    if case == 'c1':
        g = dict(load_golden('pipeline_c1.npz'))
        gen, (id1, p1, id2, p2) = c1_genome()
        keep = id1 != id2
        g.update(names=list(gen.names), length=gen.length, re_sites=gen.re_sites, id1=id1[keep], pos1=p1[keep], id2=id2[keep], pos2=p2[keep],
                 same_pairs=int(id1.sum() + p1.sum() + id2.sum() + p2.sum()) == int(g['pairs_checksum']))
        return g, [str(x) for x in g['names']]
    g = load_golden('pipeline_toy.npz' if case == 'toy' else 'pipeline_bins.npz')
    names = [str(x) for x in g['names']]
    return g, names


def pairs_text(case):
    """the fixture's read pairs as .pairs text, with a header"""
    g, names = fixture(case)
    lines = ['## pairs format v1.0\n', '#columns: readID chr1 pos1 chr2 pos2 strand1 strand2\n']
    lines += ['r{}\t{}\t{}\t{}\t{}\t+\t-\n'.format(k, names[a], x + 1, names[b], y + 1)
              for k, (a, x, b, y) in enumerate(zip(g['id1'].tolist(), g['pos1'].tolist(), g['id2'].tolist(), g['pos2'].tolist()))]
    return ''.join(lines).encode()


def sequence(case, pairs, fmt):
    import logging
    from haphic_amd import cluster
    g, names = fixture(case)
    fa_dict = {n: [None, int(l), int(r)] for n, l, r in zip(names, g['length'], g['re_sites'])}
    log = logging.FileHandler('cluster.log', mode='w')
    log.setFormatter(logging.Formatter('%(levelname)s %(message)s'))
    cluster.logger.addHandler(log)
    cluster.logger.setLevel('INFO')
    a = Args()
    if case in ('toy', 'c1'):
        frag_len_dict = {n: fa_dict[n][1] for n in names}
        Nx = set(names)
        bin_set = set()
        full, flank, HT, clm, frag_link, coord = cluster.parse_alignments_for_ctgs(
            cluster.pairs_generator(pairs, fmt), fa_dict, a, frag_len_dict, Nx, 'int32', 'int32')
        infl = (1.2, 2.0, 0.4) if case == 'toy' else (1.4, 2.2, 0.4)
    else:
        a.flank = 50
        a.remove_allelic_links = 4 if case == 'bins_allelic' else 0
        frag_names = [str(x) for x in g['frag_names']]
        frag_len_dict = {f: int(l) for f, l in zip(frag_names, g['frag_len'])}
        Nx = {f for f, x in zip(frag_names, g['frag_nx']) if x}
        bin_set = {f for f, x in zip(frag_names, g['frag_is_bin']) if x}
        split = {n for n, x in zip(names, g['split']) if x}
        full, flank, HT, clm, frag_link, coord, c2f = cluster.parse_alignments(
            cluster.pairs_generator(pairs, fmt), fa_dict, a, int(g['bin_size']), frag_len_dict, Nx, split, 'int32', 'int32')
        infl = (1.2, 2.4, 0.4)
        if a.remove_allelic_links:         # the containers thawed into real dicts, as --remove_allelic_links makes run() do
            with open('thawed.pkl', 'wb') as f:
                pickle.dump({'c2f': sorted((k, sorted(v)) for k, v in c2f.items()),
                             'coord': sorted((k, list(v)) for k, v in coord.items()),
                             'clm': sorted((k, list(v)) for k, v in clm.items()),
                             'frag_link': sorted(frag_link.items())}, f)
    cluster.output_pickle(HT, 'HT_link_dict', 'HT_links.pkl')
    cluster.output_clm(clm)
    cluster.output_pickle(full, 'full_link_dict', 'full_links.pkl')
    mat, fidx = cluster.dict_to_matrix(flank, Nx, dense_matrix=False, add_self_loops=True)
    cluster.run_mcl_clustering(mat, bin_set, frag_len_dict, fidx, 2, infl[0], infl[1], infl[2], 200, 1e-4, fa_dict, int(g['nchrs']), False)
    from haphic_amd import _lib
    _lib.files_join()
    log.close()


def main():
    case, pairs, fmt, workdir = sys.argv[1:5]
    from haphic_amd import _lib, ranks
    os.chdir(workdir)
    ctx = ranks.init()
    if ctx is None:
        _lib.check(_lib.load().hhx_set_device(0))
    return ranks.run_rank(lambda: sequence(case, pairs, fmt))


if __name__ == '__main__':
    sys.exit(main())
