"""Re-binding of the reference's own seams (SURVEY §8b S1–S6) onto the MI355X library.

    import HapHiC_cluster as H          # the unmodified reference module
    import haphic_amd.patch
    haphic_amd.patch.patch_reference(H) # then H.run(args) / HapHiC_pipeline as usual

Nothing under /root/reference is edited; the reference resolves these names at call time through its
module globals, so `setattr` on the module is all that is needed."""
from . import allelic, cluster, correct, statistics

# seam -> (reference line, replacement)
SEAMS = {
    'dot_product_mkl': ('HapHiC_cluster.py:39-43', cluster.dot_product_mkl),            # S1
    'mkl_matrix_power': ('HapHiC_cluster.py:2017-2023', cluster.mkl_matrix_power),      # S1 (keeps M^(e-1) on the device)
    'mcl': ('HapHiC_cluster.py:2026-2062', cluster.mcl),                                # S2
    'prune': ('HapHiC_cluster.py:1987-2014', cluster.prune),                            # S3
    'interpret_result': ('HapHiC_cluster.py:2065-2095', cluster.interpret_result),      # a12
    'run_mcl_clustering': ('HapHiC_cluster.py:2132-2242', cluster.run_mcl_clustering),  # S6
    'count_RE_sites': ('HapHiC_cluster.py:75-84', cluster.count_RE_sites),              # a5
    'parse_fasta': ('HapHiC_cluster.py:87-113', cluster.parse_fasta),                   # a5
    'stat_fragments': ('HapHiC_cluster.py:188-296', cluster.stat_fragments),            # a5
    'filter_fragments': ('HapHiC_cluster.py:741-940', cluster.filter_fragments),        # f1 (rank sums on the device)
    'normalize_by_nlinks': ('HapHiC_cluster.py:718-724', cluster.normalize_by_nlinks),  # a6
    'normalize_by_length': ('HapHiC_cluster.py:727-738', cluster.normalize_by_length),  # a6 (dead code in the reference)
    'reduce_inter_hap_HiC_links': ('HapHiC_cluster.py:695-707', cluster.reduce_inter_hap_HiC_links),   # a6 (GFA phasing)
}
# f2 / f3: what run() does with the S5 containers besides the seams above — the two writers (:2879, :2888, :2929) and the per-group link sums of
# output_statistics (:2354).  They only differ from the reference's functions
# for the array-backed containers of the S5 mirrors (haphic_amd/containers.py), so they travel with `ingest`.
CONTAINER_SEAMS = {
    'output_pickle': ('HapHiC_cluster.py:710-715', cluster.output_pickle),
    'output_clm': ('HapHiC_cluster.py:376-392', cluster.output_clm),
    'parse_link_dict': ('HapHiC_cluster.py:2252-2268', cluster.group_link_dict),     # per-group link sums of output_statistics :2279
}
# S4/S5: dict_to_matrix is also called in dense mode by the filters (:603) — the mirror returns `.toarray()` then;
# the device ingest returns all of the reference's containers (link tables, HT counts, CLM distance lists, first
# coordinates, ctg_pair_to_frag :1731 for split contigs + --remove_allelic_links).
OPTIONAL = {
    'dict_to_matrix': ('HapHiC_cluster.py:310-373', cluster.dict_to_matrix),
    'parse_alignments_for_ctgs': ('HapHiC_cluster.py:1596-1655', cluster.parse_alignments_for_ctgs),
    'parse_alignments': ('HapHiC_cluster.py:1658-1752', cluster.parse_alignments),
    'pairs_generator': ('HapHiC_cluster.py:1539-1559', cluster.pairs_generator),                      # a1
    'pairs_generator_inter_ctgs': ('HapHiC_cluster.py:1562-1583', cluster.pairs_generator_inter_ctgs),
    'bam_generator': ('HapHiC_cluster.py:1586-1593', cluster.bam_generator),                          # f4
}
# --correct_nrounds: what run() :2798-2851 and correct_assembly :1200-1297 (which stays the reference's code) call.  The mirrors return and
# take containers backed by the device table (haphic_amd/correct.py) and feed the S5 mirrors, so they travel with `ingest`; detect / break are
# handed the original function for containers that were thawed into plain dicts.
CORRECTION_SEAMS = {
    'parse_pairs_for_correction': ('HapHiC_cluster.py:1300-1344', correct.parse_pairs_for_correction),
    'parse_bam_for_correction': ('HapHiC_cluster.py:1362-1398', correct.parse_bam_for_correction),
    'detect_break_points': ('HapHiC_cluster.py:943-1014', correct.detect_break_points),
    'break_and_update_ctgs': ('HapHiC_cluster.py:1017-1197', correct.break_and_update_ctgs),
    'pairs_generator_for_correction_ctg': ('HapHiC_cluster.py:1401-1440', correct.pairs_generator_for_correction_ctg),
    'bam_generator_for_correction_ctg': ('HapHiC_cluster.py:1443-1470', correct.bam_generator_for_correction_ctg),
    'pairs_generator_for_correction': ('HapHiC_cluster.py:1473-1509', correct.pairs_generator_for_correction),
    'bam_generator_for_correction': ('HapHiC_cluster.py:1512-1536', correct.bam_generator_for_correction),
}
_NEEDS_ORIGINAL = ('detect_break_points', 'break_and_update_ctgs')
# --remove_allelic_links on the device tables (haphic_amd/allelic.py).  OPT-IN: the mirror works on the frozen containers of the S5 mirrors where
# the reference's function thaws them, and what patch_reference(H) does by default stays what it was.  Calls the array path does not
# serve (allelic.py lists them) go to the original function.
ALLELIC_SEAMS = {
    'remove_allelic_HiC_links': ('HapHiC_cluster.py:474-692', allelic.remove_allelic_HiC_links),
}
# output_statistics on the device tables (haphic_amd/statistics.py).  OPT-IN for the same reason: the mirror takes the per-contig numbers of every
# inflation from one call on the frozen full_link_dict's table; with the seam unbound the reference's function runs on the parse_link_dict seam above
# (cluster.group_link_dict), which also stays bound underneath for the calls the mirror hands back.
STATISTICS_SEAMS = {
    'output_statistics': ('HapHiC_cluster.py:2279-2478', statistics.output_statistics),
}
# the front of run() :2785-2831 on the device (haphic_amd/assembly.py).  OPT-IN at this level, like the seams above: parse_fasta returns rows whose
# sequences stay in HBM, parse_gfa reads every file there; stat_fragments and correct.update_bookkeeping, bound by default, work on such rows
# without reading a sequence.  Files the readers refuse go to the original functions.
FRONT_SEAMS = {
    'parse_fasta': 'HapHiC_cluster.py:87-113',
    'parse_gfa': 'HapHiC_cluster.py:150-185',
}


# position of `dense_matrix` in the reference signatures.  --dense_matrix (:2723) is the reference's own numpy mode (also what every
# install without Intel MKL runs, :2764-2768): its own convergence rule (allclose :2051), float32 trajectory, prune branch (:2003-2005) and
# interpret_result branch (:2080).  By default a seam called with dense_matrix=True is handed back to the original function
# (_dense_dispatch); patch_reference(H, dense=True) binds the device mirrors of that mode instead (cluster.prune / mcl / interpret_result /
# run_mcl_clustering with dense_matrix=True: csrc/hhx_densemcl.hip) — OPT-IN like `allelic` and `statistics`.
DENSE_ARG = {'mcl': 5, 'prune': 2, 'interpret_result': 1, 'run_mcl_clustering': 12}


def _dense_dispatch(ours, original, idx):
    def seam(*args, **kwargs):
        dense = kwargs.get('dense_matrix', args[idx] if len(args) > idx else False)
        if dense and original is not None:
            return original(*args, **kwargs)
        return ours(*args, **kwargs)
    seam.__wrapped__ = ours
    seam.__name__ = getattr(ours, '__name__', 'seam')
    seam.__doc__ = ours.__doc__
    return seam


def _with_original(ours, original):
    def seam(*args, **kwargs):
        return ours(*args, _original=original, **kwargs)
    seam.__wrapped__ = ours
    seam.__name__ = ours.__name__
    seam.__doc__ = ours.__doc__
    return seam


def _run_then_join(original):
    """run() :2738-2959 with the library's file-writer thread joined before it returns: output_pickle / output_clm of the array-backed
    containers only QUEUE HT_links.pkl, paired_links.clm and full_links.pkl (haphic_amd/csrc/hhx_jobs.hip), so the files must be complete —
    and a writer's failure raised, as the reference's own writers would raise inside run() — before the caller (main :2967,
    HapHiC_pipeline.py:358, which starts `haphic reassign` on full_links.pkl next) goes on."""
    from . import _lib

    def run(*args, **kwargs):
        try:
            out = original(*args, **kwargs)
        except BaseException:
            try:
                _lib.files_join()             # the run failed for its own reason: that one is raised, the queue is only drained
            except RuntimeError:
                pass
            raise
        _lib.files_join()
        return out
    run.__wrapped__ = original
    run.__name__ = 'run'
    run.__doc__ = original.__doc__
    return run


def patch_reference(H, ingest=True, matrix_build=True, allelic=False, statistics=False, dense=False, front=False, front_engine=None, gfa_engine=None):
    """H: the imported reference module (HapHiC_cluster).  Returns {name: original} so the caller can undo.  allelic=True (together with
    ingest): remove_allelic_HiC_links :474-692 is re-bound too (ALLELIC_SEAMS); `python -m haphic_amd cluster` asks for it on one-rank jobs.
    statistics=True (together with ingest): output_statistics :2279-2478 likewise (STATISTICS_SEAMS).  dense=True: the four seams of DENSE_ARG
    take their dense_matrix=True calls (--dense_matrix) themselves instead of handing them back to the reference's numpy code, and
    dict_to_matrix leaves the clustering matrix of a frozen table in HBM for them.  front=True (together with ingest): parse_fasta :87-113 and
    parse_gfa :150-185 are re-bound too (FRONT_SEAMS, haphic_amd/assembly.py): the sequences stay on the device behind the rows of fa_dict, and
    stat_fragments and the bookkeeping of --correct_nrounds — the mirrors bound above — count on them there; front_engine / gfa_engine: stand-ins
    for _lib.Fasta / _lib.Gfa (the tests' host engines)."""
    from . import _lib
    _lib.load()                          # fail loudly here if the HIP library is missing
    saved = {}
    seams = dict(SEAMS)
    if matrix_build:
        seams['dict_to_matrix'] = OPTIONAL['dict_to_matrix']
    if ingest:
        seams['parse_alignments_for_ctgs'] = OPTIONAL['parse_alignments_for_ctgs']
        seams['parse_alignments'] = OPTIONAL['parse_alignments']
        seams['pairs_generator'] = OPTIONAL['pairs_generator']                # a1: only together with S5, which consumes it
        seams['pairs_generator_inter_ctgs'] = OPTIONAL['pairs_generator_inter_ctgs']
        seams['bam_generator'] = OPTIONAL['bam_generator']                    # f4: consumed by the same S5 mirrors
        seams.update(CONTAINER_SEAMS)
        seams.update(CORRECTION_SEAMS)
    if ingest and allelic:
        seams.update(ALLELIC_SEAMS)
    if ingest and statistics:
        seams.update(STATISTICS_SEAMS)
    for name, (_cite, fn) in seams.items():
        saved[name] = getattr(H, name, None)
        if name in CONTAINER_SEAMS or name in _NEEDS_ORIGINAL or name in ALLELIC_SEAMS or name in STATISTICS_SEAMS:
            fn = _with_original(fn, saved[name])
        setattr(H, name, _dense_dispatch(fn, saved[name], DENSE_ARG[name]) if name in DENSE_ARG and not dense else fn)
    cluster.DENSE_SEAM_BOUND = bool(dense)
    if ingest and front:
        from . import assembly
        saved.setdefault('parse_gfa', getattr(H, 'parse_gfa', None))
        H.parse_fasta = assembly.bind_fasta(H, front_engine, original=saved['parse_fasta'])
        H.parse_gfa = assembly.bind_gfa(H, gfa_engine, original=saved['parse_gfa'])
    if ingest and getattr(H, 'run', None) is not None:
        saved['run'] = H.run
        H.run = _run_then_join(H.run)    # main() :2967 and HapHiC_pipeline.py:358 resolve `run` through the module, like every seam
    saved['INTEL_MKL'] = getattr(H, 'INTEL_MKL', None)
    H.INTEL_MKL = True                   # :2764-2768 would otherwise force the dense (numpy) mode
    return saved


def patch_reassign(R, rounds=False, engine=None, pickle=False, pickle_engine=None, resident=False, fasta=False, fasta_engine=None, gfa=False,
                   gfa_engine=None):
    """R: the imported HapHiC_reassign module.  f3: parse_link_dict :217-263 (the per-group link sums behind reassign's
    link densities) on the device for integer link counts; float / normalised links go to the original function.
    split_clm_file :581-622 (paired_links.clm routed line by line to split_clms/<group>.clm) goes through the device too
    (haphic_amd/reassign.py); the cases the reference answers with an exception of its own go to the original function.
    rounds=True: run_reassignment :266-427 and agglomerative_hierarchical_clustering :489-560 are re-bound too and parse_link_dict leaves its
    result in HBM for them (reassign.bind_rounds: what is handed back to the original functions is listed there); engine: a stand-in for
    _lib.Reassign (the tests' numpy engine), with which the three mirrors run without a GPU.  pickle=True: parse_pickle :38-50 is re-bound too
    (reassign.bind_pickle): full_links.pkl is read into arrays on the device and full_link_dict is a frozen containers.LinkTable, which the mirrors
    above consume without thawing; a file the reader does not answer goes through pickle.load.  pickle_engine: a stand-in for
    _lib.read_link_pickle (the tests' host reader).  resident=True (with pickle=True): the table stays open on the device and its keys come to
    the host only when somebody asks for the arrays; with rounds=True parse_link_dict builds its handle from it there (reassign.bind_pickle,
    reassign.bind_rounds); pickle_engine is then a stand-in for _lib.LinkPickle.open.  fasta=True: parse_fasta (HapHiC_cluster.py:87-113, imported
    :23) is re-bound too (reassign.bind_fasta): the file is parsed and its RE sites counted on the device, fa_dict is a plain dict of
    containers.FastaRow whose sequences stay there; fasta_engine: a stand-in for _lib.Fasta.  gfa=True: parse_gfa (HapHiC_cluster.py:150-185,
    imported :23, called :790) is re-bound too (assembly.bind_gfa): every file is read on the device and only the table of its S records comes to
    the host; gfa_engine: a stand-in for _lib.Gfa.  Returns {name: original}."""
    from . import reassign
    if not rounds:
        engine = None
    if engine is None or (pickle and pickle_engine is None) or (fasta and fasta_engine is None) or (gfa and gfa_engine is None):
        from . import _lib
        _lib.load()
    original = R.parse_link_dict
    original_split = R.split_clm_file
    mirrors = reassign.bind_rounds(R, engine) if rounds else {}                   # around the reference's own functions, as R holds them now

    def parse_link_dict(link_dict, ctg_group_dict, normalize_by_nlinks=False):
        return cluster.parse_link_dict(link_dict, ctg_group_dict, normalize_by_nlinks, _original=original)
    parse_link_dict.__wrapped__ = cluster.parse_link_dict
    R.parse_link_dict = parse_link_dict

    def split_clm_file(clm_file, group_ctg_dict, ctg_group_dict, subdir):
        return reassign.split_clm_file(clm_file, group_ctg_dict, ctg_group_dict, subdir, _original=original_split)
    split_clm_file.__wrapped__ = reassign.split_clm_file
    R.split_clm_file = split_clm_file
    saved = {'parse_link_dict': original, 'split_clm_file': original_split}
    if pickle:
        mirrors['parse_pickle'] = reassign.bind_pickle(R, pickle_engine, resident) if resident else reassign.bind_pickle(R, pickle_engine)
    if fasta:
        mirrors['parse_fasta'] = reassign.bind_fasta(R, fasta_engine)
    if gfa:
        from . import assembly
        mirrors['parse_gfa'] = assembly.bind_gfa(R, gfa_engine)
    for name, fn in mirrors.items():
        saved.setdefault(name, getattr(R, name))
        setattr(R, name, fn)
    return saved


# `haphic sort`: the module globals fast_sort :470-615 resolves at call time (haphic_amd/sort.py)
SORT_SEAMS = {
    'dict_to_matrix': 'HapHiC_sort.py:60-88',
    'get_density_graph': 'HapHiC_sort.py:158-192',
    'get_unfiltered_confidence_graph': 'HapHiC_sort.py:195-244',
    'filter_confidence_graph': 'HapHiC_sort.py:247-255',
    'remove_shortest_path': 'HapHiC_sort.py:456-467',
    'update': 'HapHiC_sort.py:338-437',
    'fast_sort': 'HapHiC_sort.py:470-615',          # the reference's own function, entered under sort.DEVICE_LOCK
}


# fast sorting or ALLHiC, per group (haphic_amd/sort.py bind_verdict).  OPT-IN, like `allelic` / `statistics` / `dense` above: what patch_sort(S) binds by
# default stays what it was.
SORT_VERDICT_SEAMS = {
    'compare_fast_sort_and_allhic': 'HapHiC_sort.py:645-724',
}


# each group's H/T links from HT_links.pkl (haphic_amd/sort.py bind_heads): run()'s `pickle.load` :898-901 answers an array-backed table that stays on the
# device, and get_sub_HT_dict extracts a group from it there.  OPT-IN at this level, like the verdict; `python -m haphic_amd sort` asks for it.
SORT_HEADS_SEAMS = {
    'pickle': 'HapHiC_sort.py:17 (pickle.load :898-901)',
    'get_sub_HT_dict': 'HapHiC_sort.py:117-143',
}


# the forest block of fast_sort :567-595 (haphic_amd/sort.py bind_forest).  OPT-IN at this level: patch_sort(S, forest=True); `python -m haphic_amd sort`
# asks for it unless --keep-reference-forest is given.
SORT_FOREST_SEAMS = {
    'get_unfiltered_confidence_graph': 'HapHiC_sort.py:195-244',      # no copy of the array: a token and MAXS
    'filter_confidence_graph': 'HapHiC_sort.py:247-255',              # records the cutoff; the device call filters
    'Graph': 'HapHiC_sort.py:24 (Graph(confidence_graph) :570)',
    'nxtree': 'HapHiC_sort.py:25 (nxtree.maximum_spanning_tree :570)',
    'shortest_path': 'HapHiC_sort.py:24 (dict(shortest_path(tree))[source][target] :590)',
}


def patch_sort(S, engine=None, verdict=False, verdict_engine=None, heads=False, heads_engine=None, forest=False):
    """S: the imported HapHiC_sort module.  The dense work of fast sorting goes to the device (haphic_amd/sort.py); fast_sort, the spanning forest,
    split_new_scaffold, the .tour writer, the ALLHiC child and run() stay the reference's.  run() :875-876 forks a multiprocessing.Pool: a process
    that has initialised the GPU must not be forked into workers that use it, so S.Pool becomes the ThreadPool (same apply_async / close / join);
    one lock serialises the device part across its threads, the ALLHiC children run beside it.  engine: a stand-in for _lib.SortGraph (the tests'
    numpy engine).  verdict=True: compare_fast_sort_and_allhic :645-724 (which tour final_tours/<group>.tour links to) is re-bound too: the weighted-LIS
    sums of all rotations come from one library call; verdict_engine: a stand-in for _lib.sort_verdict_sums (the tests' host engine); `python -m
    haphic_amd sort` asks for it.  heads=True: S.pickle becomes a proxy of the pickle module whose load() reads HT_links.pkl into arrays on the device
    (run() :898-901) and get_sub_HT_dict :117-143 is re-bound to extract every group from them there (SORT_HEADS_SEAMS; sort.bind_heads lists what
    goes to the reference's function); heads_engine: a stand-in for _lib.LinkPickle.open (the tests' host reader).  forest=True: the forest block
    :567-595 runs on the device too (SORT_FOREST_SEAMS; sort.bind_forest lists what goes back to the reference's block); the engine needs
    confidence_device / forest / fetch_confidence, with one that has no forest() every round is the reference's.  Returns {name: original}."""
    from multiprocessing.pool import ThreadPool
    from . import sort
    if engine is None or (verdict and verdict_engine is None):
        from . import _lib
        _lib.load()
    mirrors = sort.bind(S, engine)
    assert set(mirrors) == set(SORT_SEAMS)
    if verdict:
        mirrors['compare_fast_sort_and_allhic'] = sort.bind_verdict(S, verdict_engine)
    saved = {name: getattr(S, name) for name in mirrors}
    saved['Pool'] = S.Pool
    for name, fn in mirrors.items():
        setattr(S, name, fn)
    S.Pool = ThreadPool
    if forest:
        saved.update(patch_sort_forest(S))
    if heads:
        saved.update(patch_sort_heads(S, heads_engine))
    return saved


def patch_sort_forest(S):
    """The seams of SORT_FOREST_SEAMS alone, for a module patch_sort has been applied to (patch_sort(S, forest=True) ends here; the wrapper command
    calls it after patch_sort unless --keep-reference-forest is given).  Returns {name: what
    was bound before} for the names patch_sort has not saved yet."""
    from . import sort
    mirrors = sort.bind_forest(S)
    assert set(mirrors) == set(SORT_FOREST_SEAMS)
    saved = {name: getattr(S, name, None) for name in ('Graph', 'nxtree', 'shortest_path')}
    for name, fn in mirrors.items():
        setattr(S, name, fn)
    return saved


def patch_sort_heads(S, engine=None):
    """The two seams of SORT_HEADS_SEAMS alone (patch_sort(S, heads=True) ends here; the wrapper command calls it after patch_sort unless
    --keep-reference-heads is given).  Returns {name: original}."""
    from . import sort
    if engine is None:
        from . import _lib
        _lib.load()
    saved = {name: getattr(S, name, None) for name in SORT_HEADS_SEAMS}
    S.pickle, S.get_sub_HT_dict = sort.bind_heads(S, engine)
    return saved


# `haphic build`: the two module globals run() :244-283 resolves at call time (haphic_amd/scaffolds.py)
BUILD_SEAMS = {
    'parse_fasta': 'HapHiC_cluster.py:87-113',           # bound into HapHiC_build by `from HapHiC_cluster import parse_fasta` :17
    'build_final_scaffolds': 'HapHiC_build.py:74-179',
}


def patch_build(B, engine=None):
    """B: the imported HapHiC_build module.  parse_fasta reads the FASTA file on the device and returns a containers.FastaTable, whose sequences
    stay in HBM; build_final_scaffolds writes scaffolds.fa from them with one library call and both AGP files from the host arrays
    (haphic_amd/scaffolds.py, which lists what is handed back to the reference's own functions).  parse_tours, parse_corrected_ctgs,
    generate_juicebox_script and run() stay the reference's.  engine: a stand-in for _lib.Fasta (the tests' numpy engine).  Returns {name: original}."""
    from . import scaffolds
    if engine is None:
        from . import _lib
        _lib.load()
    saved = {name: getattr(B, name) for name in BUILD_SEAMS}
    original_fasta, original_build = saved['parse_fasta'], saved['build_final_scaffolds']

    def parse_fasta(fasta, RE='GATC', keep_letter_case=False, logger=B.logger):
        return scaffolds.parse_fasta(fasta, RE, keep_letter_case, logger, _original=original_fasta, _engine=engine)
    parse_fasta.__wrapped__ = scaffolds.parse_fasta
    B.parse_fasta = parse_fasta

    def build_final_scaffolds(tour_dict, fa_dict, output_ctgs, corrected_ctg_set, args):
        return scaffolds.build_final_scaffolds(tour_dict, fa_dict, output_ctgs, corrected_ctg_set, args, _original=original_build, _logger=B.logger)
    build_final_scaffolds.__wrapped__ = scaffolds.build_final_scaffolds
    B.build_final_scaffolds = build_final_scaffolds
    return saved


# `haphic refsort`: the three module globals run() :383-412 resolves at call time (haphic_amd/refsort.py)
REFSORT_SEAMS = {
    'parse_fasta': 'HapHiC_cluster.py:87-113',           # bound into HapHiC_refsort by `from HapHiC_cluster import parse_fasta` :16
    'parse_paf': 'HapHiC_refsort.py:81-134',
    'order_and_orient_groups': 'HapHiC_refsort.py:151-342',
}


def patch_refsort(F, engine=None, paf=True):
    """F: the imported HapHiC_refsort module.  parse_fasta reads the FASTA file on the device and returns a containers.FastaTable (the mirror
    patch_build binds); parse_paf reads the PAF file on the device and builds the reference's nested dict from the table with numpy;
    order_and_orient_groups takes both find_lis sums of all groups from one library call, prints the AGP lines from host code and writes the FASTA
    records by one library call on the path fout.name (haphic_amd/refsort.py, which lists what is handed back to the reference's own functions).
    parse_agp, get_max_ovl_group, alignment_check and run() stay the reference's.  engine: a stand-in for the _lib module with Fasta, Paf,
    lis_sums and LisUnsupported (the tests' numpy engine).  paf=False leaves parse_paf the reference's (the wrapper's default, which follows
    profiles/refsort_bench.json); order_and_orient_groups flattens the reference's dict as it does the mirror's.  Returns {name: original}."""
    from . import refsort, scaffolds
    from .containers import FastaTable
    if engine is None:
        from . import _lib
        _lib.load()
    saved = {name: getattr(F, name) for name in REFSORT_SEAMS}
    original_fasta, original_paf, original_order = saved['parse_fasta'], saved['parse_paf'], saved['order_and_orient_groups']
    refsort.STATS.clear()

    def parse_fasta(fasta, RE='GATC', keep_letter_case=False, logger=F.logger):
        out = scaffolds.parse_fasta(fasta, RE, keep_letter_case, logger, _original=original_fasta, _engine=None if engine is None else engine.Fasta)
        refsort.STATS['parse_fasta'] = 'device' if isinstance(out, FastaTable) else 'reference'
        return out
    parse_fasta.__wrapped__ = scaffolds.parse_fasta
    F.parse_fasta = parse_fasta

    def parse_paf(paf, ctg_group_dict, aln_len_cutoff):
        return refsort.parse_paf(paf, ctg_group_dict, aln_len_cutoff, _original=original_paf, _engine=engine, _logger=F.logger)
    parse_paf.__wrapped__ = refsort.parse_paf
    if paf:
        F.parse_paf = parse_paf

    def order_and_orient_groups(ctg_group_dict, group_ref_dict, group_agp_lines, group_len_dict, one_ctg_groups, args, fa_dict=None, fout=None):
        return refsort.order_and_orient_groups(ctg_group_dict, group_ref_dict, group_agp_lines, group_len_dict, one_ctg_groups, args, fa_dict, fout,
                                               _original=original_order, _engine=engine, _logger=F.logger)
    order_and_orient_groups.__wrapped__ = refsort.order_and_orient_groups
    F.order_and_orient_groups = order_and_orient_groups
    return saved


def unpatch_reference(H, saved):
    cluster.DENSE_SEAM_BOUND = False
    for name, fn in saved.items():
        if fn is None and hasattr(H, name):
            delattr(H, name)
        elif fn is not None:
            setattr(H, name, fn)
