"""`python -m haphic_amd cluster <arguments of "haphic cluster">` — HapHiC's own step 1 with the MI355X library behind
its seams (SURVEY §8b "who calls it"): import the reference's HapHiC_cluster module, re-bind S1-S6 with
haphic_amd.patch.patch_reference, call the reference's run(args, log_file) exactly as its main() does (:2962-2967).
Argument parsing, logging, file formats and every stage outside the hot path are the reference's own code.
`--correct_nrounds N` (assembly correction) runs on the device too: both passes over the alignment file, the break-point detection and the breaking
(haphic_amd/correct.py); correct_assembly's round loop and its FASTA writer stay the reference's.
`python -m haphic_amd plot <arguments of "haphic plot">` does the same for HapHiC_plot.py: parse_pairs / parse_bam (the read-pair
binning into the scaffold-bin contact matrix) and normalize_matrix (the Knight-Ruiz balancing of `--normalization KR`, the scaled
matrix and the median behind vmax; `log10` / `none`: the median alone) run on the device (haphic_amd.plot.patch_plot), main() is the reference's.
`python -m haphic_amd reassign <arguments of "haphic reassign">` wraps HapHiC_reassign.py: parse_link_dict (the per-group link sums) and
split_clm_file (paired_links.clm split into split_clms/<group>.clm, haphic_amd/reassign.py) run on the device (haphic_amd.patch.patch_reassign),
and so do the rescue and reassignment rounds (run_reassignment :266-427) and the group-pair sums of the agglomerative step (:489-560) between them
(patch_reassign(R, rounds=True)); the front of run() — parse_fasta, parse_pickle and the preparation of parse_link_dict — stays on the device as well
(fasta=True, pickle=True, resident=True); run() :752-916 is the reference's, called as its main() :919-924 calls it.
`python -m haphic_amd sort <arguments of "haphic sort">` wraps HapHiC_sort.py: the dense work of fast sorting (link matrix, density graph, confidence
graph and the link re-aggregation of every round, haphic_amd/sort.py) runs on the device (haphic_amd.patch.patch_sort), and so does the forest block of every round (:567-595: filter, maximum spanning forest, the position of every node
along its path; patch_sort(S, forest=True)), from which the host builds the small networkx graph that settles the order and direction of the paths;
fast_sort's loop, the ALLHiC child per group and run() :847-959 are the reference's, its process pool replaced by threads; called as its main() :962-967 does.
The front of run() :898-923 runs on the device too: HT_links.pkl is read into arrays that stay there and each group's sub_HT_dict / HT_index_dict
(get_sub_HT_dict :117-143) comes from two streaming passes over them and a sort of the survivors (patch_sort(S, heads=True)).  `sort` with nothing after it has nothing to hand on and exits with a usage message.
`python -m haphic_amd build <arguments of "haphic build">` wraps HapHiC_build.py: parse_fasta (HapHiC_cluster.py:87-113: the FASTA text goes to HBM in one piece
and is compacted there into the contigs' sequences, haphic_amd/scaffolds.py) and build_final_scaffolds :74-179 (scaffolds.fa gathered, reverse-complemented and
wrapped on the device, written slab by slab; both AGP files from the host arrays) run on the device (haphic_amd.patch.patch_build); parse_tours, the juicebox
script and run() :244-283 are the reference's, called as its main() :286-291 calls it.
`python -m haphic_amd refsort <arguments of "haphic refsort">` wraps HapHiC_refsort.py: parse_fasta as for `build`; parse_paf :81-134 (the PAF file goes to HBM in
one piece, the first 12 fields of every line are located there whatever the length of its cg:Z: tag, csrc/hhx_paf.hip, and the nested dict is built from the
table with numpy); order_and_orient_groups :151-342 (both weighted longest-increasing-subsequence sums of all groups from one device call, csrc/hhx_sortverdict.hip
hhx_lis_sums; the AGP lines from host code; scaffolds.refsort.fa sliced, reverse-complemented and wrapped on the device and written slab by slab to the PATH of
--fout, haphic_amd/refsort.py) run on the device (haphic_amd.patch.patch_refsort; parse_paf only with --device-paf); parse_agp, alignment_check and run() :383-412 are the reference's, called as its
main() :415-420 calls it.

The reference checkout is found through --reference DIR or $HAPHIC_REFERENCE (the repository root or its scripts/
directory).  Extra flags of the wrapper (removed before the reference parses the command line):
  --device N                 HIP device ordinal (default 0)
  --keep-reference-ingest    leave S5 / a1 (parse_alignments*, pairs_generator*) and the correction passes to the reference
  --keep-reference-allelic   cluster only: leave --remove_allelic_links N (remove_allelic_HiC_links :474-692) to the reference's per-key loops, which
                             thaw full_link_dict, flank_link_dict and ctg_coord_dict into Python dicts first.  Without the flag a one-rank job
                             takes the concordance ratios and the verdict on the device tables (haphic_amd/allelic.py); under --gpus N > 1 or
                             torchrun the reference's loops run whatever the flag says (the sharded tables are not served).  The device path
                             also hands a call back to the reference's function when the containers were already thawed, flank_link_dict is
                             empty, --remove_concentrated_links or ultra-long reads (--ul) are on, the log level is DEBUG (the per-key debug
                             lines), a contig is shorter than --nwindows bp, or --max_read_pairs exceeds 4096
  --keep-reference-rounds    reassign only: leave run_reassignment :266-427 and agglomerative_hierarchical_clustering :489-560 to the reference's loops
                             over Python dicts, which parse_link_dict then builds as before.  Without the flag parse_link_dict leaves the
                             per-(contig, group) cells in device memory, every round is a chain of kernel launches on them and only the changed
                             values are written back into ctg_group_dict and group_RE_dict.  A call still goes to the reference's function when
                             the link counts are floats or --normalize_by_nlinks is on, a whitelist is given, --min_links is below 1, the log
                             level is DEBUG (the per-contig lines), a link or RE total reaches 2^53, or the cells of contigs x groups do not
                             fit in half of the device's memory
  --keep-reference-pickle    reassign only: leave parse_pickle :38-50 to pickle.load, which builds full_link_dict as a Python dict of every key of
                             full_links.pkl (tens of GB of objects at 100k contigs) that parse_link_dict then flattens again.  Without the flag the
                             file is read into arrays on the device (csrc/hhx_pickleread.hip) and full_link_dict is an array-backed table that
                             parse_link_dict, the rounds and the agglomerative step consume without turning it into a dict.  A file still goes through
                             pickle.load when it is not a protocol 4 / 5 pickle of a collections.defaultdict(int), holds any opcode besides names of
                             at most 255 bytes, 2-tuples, integers of at most 64 bits and floats in MARK .. SETITEMS / SETITEM batches (3-tuple keys,
                             True / None values, 2^63 ...), refers to a memo slot that holds no name, writes a key twice, ends early, has bytes
                             after STOP or frames that do not tile it, mixes floats with integers beyond 2^53, or is larger than half of the
                             device's memory
  --keep-reference-fasta     reassign only: leave parse_fasta (HapHiC_cluster.py:87-113) to the reference's per-line loop, which joins every sequence
                             into a Python string and counts its RE sites one contig after the other.  Without the flag the file is parsed and the RE
                             sites of all contigs are counted on the device (csrc/hhx_fasta.hip, csrc/hhx_resites.hip) and fa_dict is a plain dict
                             whose rows hold length and RE sites; a row copies its sequence from the device only if something reads it (run() never
                             does).  The reference's function still takes a file with a byte >= 0x80, with a sequence line before the first header,
                             with repeated contig names, or beyond half of the device's memory
  --device-front             cluster only, OPT-IN (tools/cluster_front_bench.py has not been run at full size yet; the default follows its record):
                             run the front of run() :2785-2831 on the device.  The FASTA file is parsed there and the rows of fa_dict carry views of
                             the sequences that stay there (haphic_amd/assembly.py): stat_fragments counts the bins and flanks of all contigs in one
                             call on them, the children of a --correct_nrounds round are views counted in one call, and only corrected_asm.fa
                             :1267-1269 reads sequences (one copy of all of them); every GFA file (--gfa) is read on the device (csrc/hhx_gfa.hip) and
                             only the table of its S records comes to the host.  Without the flag parse_fasta is the per-line loop, which joins every
                             sequence into a Python string, stat_fragments and the correction slice those strings and copy them to the device to
                             count RE sites, and parse_gfa is the reference's per-line loop.  parse_fasta hands back what --keep-reference-fasta
                             lists; parse_gfa hands the whole call to the reference's function when a file has an S record with fewer than five
                             fields, an integer that is not 1 to 18 digits, a name beyond 255 bytes, a byte >= 0x80, is larger than half of the
                             device's memory or is no regular file.  No effect with --keep-reference-ingest
  --device-gfa               reassign only, OPT-IN for the same reason: read the files of --gfa (parse_gfa, HapHiC_cluster.py:150-185) on the device as
                             --device-front does; the same files go back to the reference's function
  --keep-host-keys           reassign only: copy the keys of full_links.pkl to the host after reading, as parse_link_dict's host passes over them
                             need (renumbering, the check for a key that names one contig twice, the total).  Without the flag the table stays open
                             on the device, those checks are one pass over the keys there and the handle of the rounds is built from them by
                             device-to-device copies; the keys come to the host only if something turns full_link_dict into a dict.  Tables with a
                             float or negative value, a key that names one contig twice or totals beyond 2^52 take the host passes as before.  No
                             effect with --keep-reference-pickle or --keep-reference-rounds
  --keep-reference-statistics  cluster only: leave output_statistics :2279-2478 (the *_statistics.txt files and statistics.pdf of every inflation) to the
                             reference's per-contig loop over ctg_group_link_dict, which is rebuilt as Python dicts once per inflation.  Without the
                             flag a one-rank job takes the per-contig numbers of all inflations from one device call on the frozen full_link_dict
                             (haphic_amd/statistics.py) and writes the same bytes; under --gpus N > 1 or torchrun the reference's loop runs whatever
                             the flag says.  The device path also hands the call back when full_link_dict was thawed or holds float values
                             (--remove_concentrated_links, GFA phasing) or a contig has no RE site
  --keep-reference-dense     cluster only: leave --dense_matrix (:2723; the reference's numpy mode of prune / mcl / interpret_result / run_mcl_clustering, with its
                             own convergence rule allclose :2051) to the reference's numpy code on the host.  Without the flag a one-rank job with
                             --dense_matrix runs that recurrence on the device (float32 MFMA products, csrc/hhx_densemcl.hip): same round counts and
                             clusters, the n x n matrix never leaves HBM; under --gpus N > 1 or torchrun the numpy code runs whatever the flag says.
                             Without --dense_matrix the flag changes nothing
  --keep-reference-build     build only: leave parse_fasta and build_final_scaffolds to the reference's per-line and per-60-bases Python loops.  Without the
                             flag a call still goes to the reference's function for a FASTA file with a byte >= 0x80, with a sequence line in front of
                             the first header, with a contig name that repeats, or beyond half of the device's memory, and for --max_width < 1 or --Ns < 0
  --keep-reference-refsort   refsort only: leave parse_fasta, parse_paf and order_and_orient_groups to the reference's loops (line.split() over every cg:Z: tag, two
                             O(n^2) find_lis passes per group in Python, 60 bases per fout.write).  Without the flag parse_fasta and
                             order_and_orient_groups run on the device; a call still goes to the reference's function, whole and before it logs a
                             line, for a FASTA file as --keep-reference-build lists; for --max_width < 1, an AGP slice that is not
                             1 <= start <= end <= len(contig), a negative N count, an orientation that is neither + nor -, a group of more than 2^18
                             alignments, an alignment length <= 0, a group_ref_dict that does not flatten into arrays
  --device-paf               refsort only, OPT-IN: run parse_paf on the device too.  Measured (tools/refsort_bench.py, profiles/refsort_bench.json): at 3 Gb /
                             940 500 lines 0.22 s against the reference's 2.4 s (bare) and 0.41 s against 7.6 s (2.9 GB of text with cg:Z: tails), but at
                             30 Mb / 9 405 lines its slowest repeats, 14 and 27 ms, stand against 15 and 51 ms of the reference measured on another box: not
                             the factor of 2 the rule asks of a yardstick from another box, so the piece stays opt-in.  With the flag a file still goes
                             to the reference's function for a line of fewer than 12 fields, an integer field that is not 1 to 18 digits, a name beyond
                             255 bytes, a byte >= 0x80, a coordinate of 2^52 or more, beyond half of the device's memory or when it is no regular file
  --keep-reference-verdict   sort only: leave compare_fast_sort_and_allhic :645-724 (fast sorting or ALLHiC, per group) to the reference's loop: for each of the
                             n - 1 rotations of the fast-sort tour two O(n^2) weighted longest-increasing-subsequence passes in Python.  Without the flag the
                             sums of all rotations come from one device call (haphic_amd/sort.py bind_verdict: one wavefront per rotation, csrc/hhx_sortverdict.hip)
                             and the ratio rule, the threshold and the log lines stay in Python: same verdict, same log line.  A call still goes to the
                             reference's function for a group of one contig, an ALLHiC tour that is no permutation of the fast-sort tour, a length that
                             is not a non-negative int, and beyond 2^18 contigs
  --keep-reference-heads     sort only: leave the front of run() :898-923 to the reference: pickle.load builds HT_link_dict as a Python dict of every key of
                             HT_links.pkl (tens of GB of objects at 100k contigs) and get_sub_HT_dict :117-143 does four dict look-ups for every pair of
                             contigs of every group.  Without the flag the file is read into arrays on the device (csrc/hhx_pickleread.hip), HT_link_dict is
                             an array-backed table that stays there, and each group's sub_HT_dict comes from two streaming passes over those arrays (haphic_amd/sort.py
                             bind_heads): the same items and HT_index_dict in the same order, the same tour files.  `del HT_link_dict` :922 frees the
                             device memory.  A file still goes through pickle.load when the reader does not answer it (as --keep-reference-pickle lists),
                             and a group goes to the reference's function — on the table turned into the dict pickle.load gives — when a contig is listed
                             twice, the table holds float values, or 2 n is beyond int32
  --keep-reference-forest    sort only: leave the forest block of every round of fast_sort (:567-595) to the reference: the 8 * shape^2 byte confidence array is
                             copied to the host, networkx.Graph() scans all its cells in Python, Kruskal sorts tuples and shortest_path computes all pairs of
                             every tree to read one path.  Without the flag the array stays on the device, one call filters it and builds the maximum
                             spanning forest with every node's tree and position along its path (haphic_amd/sort.py bind_forest, csrc/hhx_sort.hip), and the
                             host builds the networkx graph of the chosen edges alone, asks networkx for the components and their ends, and reads each path
                             off the positions: the same paths in the same order and direction, the same tour files and log lines.  A round still goes to
                             the reference's block, on the array fetched from the device, when its forest is no set of paths (a cutoff below 1 can fork a
                             tree; the reference then fails its assert as before), when the group runs the reference's functions already (as
                             dict_to_matrix decides in round 1, or after foreign code touched its sub_HT_dict or the confidence token), beyond shape
                             65535, and when maximum_spanning_tree is called with anything but algorithm='kruskal'
  --stub-missing-imports     development boxes only: empty stand-ins for pysam / portion when they are not installed
                             (the .pairs path needs neither; BAM input then fails loudly inside the reference); for refsort the stand-in of
                             portion is haphic_amd/intervals.py, closed intervals that work, because the calls handed back build them
  --gpus N                   cluster only: run the job as N ranks, one fresh process per rank (haphic_amd/ranks.py); the files are
                             byte-identical to the one-rank run; with --correct_nrounds both correction passes over a .pairs file are shared
                             across the ranks too.  Under torchrun (RANK / WORLD_SIZE set) its ranks are used instead.
  --host-transport           with --gpus: gloo through host memory instead of RCCL, for ranks that share a device (the default when N
                             exceeds the number of devices)
"""
import os
import sys
import types


def _take(argv, flag, has_value):
    if flag not in argv:
        return None
    k = argv.index(flag)
    if not has_value:
        del argv[k]
        return True
    if k + 1 >= len(argv):
        raise SystemExit('{} needs a value'.format(flag))
    value = argv[k + 1]
    del argv[k:k + 2]
    return value


def _reference_scripts(path):
    for cand in (path, os.path.join(path or '', 'scripts')):
        if cand and os.path.isfile(os.path.join(cand, 'HapHiC_cluster.py')):
            return cand
    raise SystemExit('HapHiC checkout not found: pass --reference DIR or set HAPHIC_REFERENCE (looked for HapHiC_cluster.py in {!r})'.format(path))


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ('-h', '--help'):
        print(__doc__)
        return 0
    command = argv.pop(0)
    if command not in ('cluster', 'plot', 'reassign', 'sort', 'build', 'refsort'):
        raise SystemExit('haphic_amd wraps the "cluster", "plot", "reassign", "sort", "build" and "refsort" steps only (got {!r}); run the other steps with the reference'.format(command))
    if command == 'sort' and not argv:
        # nothing to hand to the reference: say what the wrapper is, as for a step it does not wrap, rather than go looking for the checkout
        raise SystemExit('haphic_amd wraps the "cluster", "plot", "reassign", "sort" and "build" steps only and hands them the arguments of the reference\'s '
                         'command; {!r} came without any (haphic sort: fasta HT_links clm_dir groups ...)'.format(command))
    from . import ranks
    gpus, host_transport = ranks.take_args(argv)
    if command in ('plot', 'reassign', 'sort', 'build', 'refsort') and (gpus or 1) > 1:
        raise SystemExit('--gpus is a flag of the "cluster" step only')
    if (gpus or 1) > 1 and not ranks.in_torchrun():
        # one fresh child process per rank (never exec: this process may not replace itself), each with RANK / WORLD_SIZE / LOCAL_RANK
        return ranks.launch([sys.executable, '-m', 'haphic_amd', command] + argv, gpus, host_transport)
    ref = _take(argv, '--reference', True) or os.environ.get('HAPHIC_REFERENCE')
    device = int(_take(argv, '--device', True) or 0)
    keep_ingest = bool(_take(argv, '--keep-reference-ingest', False))
    keep_allelic = bool(_take(argv, '--keep-reference-allelic', False))
    keep_statistics = bool(_take(argv, '--keep-reference-statistics', False))
    keep_dense = bool(_take(argv, '--keep-reference-dense', False))
    keep_rounds = bool(_take(argv, '--keep-reference-rounds', False))
    keep_pickle = bool(_take(argv, '--keep-reference-pickle', False))
    keep_fasta = bool(_take(argv, '--keep-reference-fasta', False))
    keep_host_keys = bool(_take(argv, '--keep-host-keys', False))
    keep_build = bool(_take(argv, '--keep-reference-build', False))
    keep_refsort = bool(_take(argv, '--keep-reference-refsort', False))
    device_paf = bool(_take(argv, '--device-paf', False))
    keep_verdict = bool(_take(argv, '--keep-reference-verdict', False))
    keep_heads = bool(_take(argv, '--keep-reference-heads', False))
    keep_forest = bool(_take(argv, '--keep-reference-forest', False))
    device_front = bool(_take(argv, '--device-front', False))
    device_gfa = bool(_take(argv, '--device-gfa', False))
    stub = bool(_take(argv, '--stub-missing-imports', False))
    scripts = _reference_scripts(ref)
    if stub:
        for name, attrs in (('pysam', {'set_verbosity': lambda *a, **k: None, 'AlignmentFile': None}), ('portion', {'closed': None, 'empty': None})):
            try:
                __import__(name)
            except ImportError:
                m = types.ModuleType(name)
                m.__dict__.update(attrs)
                if name == 'portion' and command == 'refsort':       # the calls handed back to the reference build intervals (:72, :229)
                    from . import intervals
                    m.closed = intervals.closed
                sys.modules[name] = m
    from . import _lib, patch
    _lib.check(_lib.load().hhx_set_device(device))                 # fails here, loudly, without a GPU or the library
    ctx = ranks.init(True if host_transport else None) if command == 'cluster' else None     # a rank of a multi-rank job: its own device
    if ctx is not None and ctx.rank > 0:
        return ranks.run_rank(None)                                 # serve the phases rank 0 announces; rank 0 writes every file
    sys.path.insert(0, scripts)
    if command == 'plot':
        import HapHiC_plot as P                                     # needs pysam / portion / matplotlib, as the reference does
        from . import plot
        plot.patch_plot(P)
        sys.argv = ['haphic plot'] + argv
        P.main()
        return 0
    if command == 'reassign':
        import HapHiC_reassign as R                                 # needs pysam / sklearn, as the reference does
        patch.patch_reassign(R, rounds=not keep_rounds, pickle=not keep_pickle, resident=not (keep_pickle or keep_rounds or keep_host_keys),
                             fasta=not keep_fasta, gfa=device_gfa)
        sys.argv = ['haphic reassign'] + argv
        R.run(R.parse_arguments(), 'HapHiC_reassign.log')           # == HapHiC_reassign.main() :919-924
        return 0
    if command == 'sort':
        import HapHiC_sort as S                                     # needs networkx / scipy, as the reference does
        from . import sort
        sort.DEVICE = device                                        # the pool's threads select it before their first call
        patch.patch_sort(S, verdict=not keep_verdict)
        if not keep_forest:
            patch.patch_sort_forest(S)                              # == patch_sort(S, ..., forest=True)
        if not keep_heads:
            patch.patch_sort_heads(S)                               # == patch_sort(S, ..., heads=True)
        sys.argv = ['haphic sort'] + argv
        S.run(S.parse_arguments(), 'HapHiC_sort.log')               # == HapHiC_sort.main() :962-967
        return 0
    if command == 'build':
        import HapHiC_build as B                                    # imports HapHiC_cluster for parse_fasta :17, with all it needs
        if not keep_build:
            patch.patch_build(B)
        sys.argv = ['haphic build'] + argv
        B.run(B.parse_arguments(), 'HapHiC_build.log')              # == HapHiC_build.main() :286-291
        return 0
    if command == 'refsort':
        import HapHiC_refsort as F                                  # imports HapHiC_cluster for parse_fasta :16, with all it needs
        if not keep_refsort:
            patch.patch_refsort(F, paf=device_paf)                  # parse_paf: opt-in, as profiles/refsort_bench.json decides
        sys.argv = ['haphic refsort'] + argv
        F.run(F.parse_arguments(), 'HapHiC_refsort.log')            # == HapHiC_refsort.main() :415-420
        return 0
    import HapHiC_cluster as H                                      # the unmodified reference module
    patch.patch_reference(H, ingest=not keep_ingest, allelic=not keep_allelic and ctx is None,      # the allelic, statistics and dense seams: one-rank jobs only
                          statistics=not keep_statistics and ctx is None, dense=not keep_dense and ctx is None,
                          front=device_front)                       # rank 0 alone runs the front; the other ranks never see fa_dict
    sys.argv = ['haphic cluster'] + argv
    return ranks.run_rank(lambda: H.run(H.parse_arguments(), 'HapHiC_cluster.log'))      # == HapHiC_cluster.main() :2962-2967


if __name__ == '__main__':
    sys.exit(main())
