"""One rank of a multi-rank `haphic cluster --correct_nrounds 2` job over a .pairs file, for tests/test_gpu_ranks_correction.py: run()'s seam
sequence with the assembly correction in front (:2829-2945 — parse_fasta, pass one, the rounds of correct_assembly :1204-1243 driven as
tests/correction_fixture.check_against_mirrors drives them, the corrected FASTA, stat_fragments on the corrected contigs, pass two through the
correction-aware generator or, when nothing was broken, the ordinary one, the link files, the sweep) on rank 0, ranks.serve() on the others.
Started by ranks.launch() with RANK / WORLD_SIZE set:

    python tests/ranks_correction_job.py CASE FASTA PAIRS FORMAT WORKDIR

    CASE  ctg      contigs stay whole: pairs_generator_for_correction_ctg -> parse_alignments_for_ctgs
          bins     --bin_size splits them: pairs_generator_for_correction -> parse_alignments
          nobreak  a region cut-off no contig reaches: no break point, the ordinary generators (:2862-2873)
          tiny     as ctg, for a file of a few lines: the job ends with the link files (nothing to cluster)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NCHRS = 3
INFLATIONS = (1.2, 2.0, 0.4)


def sequence(case, fasta, pairs, fmt):
    from haphic_amd import _lib, cluster, correct
    from tests import correction_fixture
    fx = correction_fixture.load()
    args = correction_fixture._args(fx, 2)
    args.alignments, args.aln_format, args.fasta = pairs, fmt, fasta
    args.nwindows, args.skip_clustering = 50, False
    if case == 'nobreak':
        args.min_region_cutoff = 10 ** 9
    fa = cluster.parse_fasta(fasta, RE=args.RE)
    # ---- correct_assembly :1200-1297
    cov_d, pos_d = correct.parse_pairs_for_correction(fa, args)
    unbroken, source, fpos, ffrag = set(fa), {}, {}, {}
    for rnd in range(args.correct_nrounds):
        bp = correct.detect_break_points(cov_d, fa, args)
        if not bp:
            break
        if rnd == 0:
            for c in bp:
                source[c], fpos[c], ffrag[c] = c, [0], [c]
        correct.break_and_update_ctgs(bp, pos_d, cov_d, source, fpos, ffrag, fa, {}, unbroken, args, rnd + 1 == args.correct_nrounds)
        unbroken -= set(bp)
    del cov_d, pos_d
    with open('corrected_asm.fa', 'w') as f:
        for name, info in fa.items():
            f.write('>{}\n{}\n'.format(name, info[0]))
    with open('corrected_ctgs.txt', 'w') as f:
        f.write(''.join(name + '\n' for name in fa if name not in unbroken))
    # ---- run() :2835-2945 on the corrected contigs
    bin_size = int(fx['meta']['bin_size_kb']) if case == 'bins' else 0
    _sorted, bin_set, bin_bp, frag_len_dict, nx, _re, split_set = cluster.stat_fragments(fa, args.RE, {}, set(), nchrs=NCHRS, flank=args.flank, Nx=100,
                                                                                         bin_size=bin_size)
    assert bool(split_set) == (case == 'bins')
    if split_set:
        aln = correct.pairs_generator_for_correction(pairs, fmt, fpos, ffrag) if fpos else cluster.pairs_generator(pairs, fmt)
        full, flank, HT, clm, _frag_link, _coord, _c2f = cluster.parse_alignments(aln, fa, args, bin_bp, frag_len_dict, nx, split_set, 'int32', 'int32')
    else:
        aln = correct.pairs_generator_for_correction_ctg(pairs, fmt, fpos, ffrag) if fpos else cluster.pairs_generator_inter_ctgs(pairs, fmt)
        full, flank, HT, clm, _frag_link, _coord = cluster.parse_alignments_for_ctgs(aln, fa, args, frag_len_dict, nx, 'int32', 'int32')
    cluster.output_pickle(HT, 'HT_link_dict', 'HT_links.pkl')
    cluster.output_clm(clm)
    cluster.output_pickle(full, 'full_link_dict', 'full_links.pkl')
    if case != 'tiny':
        mat, fidx = cluster.dict_to_matrix(flank, nx, dense_matrix=False, add_self_loops=True)
        cluster.run_mcl_clustering(mat, bin_set, frag_len_dict, fidx, 2, INFLATIONS[0], INFLATIONS[1], INFLATIONS[2], 200, 1e-4, fa, NCHRS, False)
    _lib.files_join()
    with open('broken.txt', 'w') as f:                     # what the correction did, for the test to look at
        f.write('{}\n'.format(len(fpos)))


def main():
    case, fasta, pairs, fmt, workdir = sys.argv[1:6]
    from haphic_amd import _lib, ranks
    os.chdir(workdir)
    ctx = ranks.init()
    if ctx is None:
        _lib.check(_lib.load().hhx_set_device(0))
    return ranks.run_rank(lambda: sequence(case, fasta, pairs, fmt))


if __name__ == '__main__':
    sys.exit(main())
